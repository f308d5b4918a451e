"""GPU: the three entries of include/grf_svgp.h called directly, at edge shapes.

grf_robustmax_ve_f64 and grf_robustmax_predict_f64 at n in {1, 2, 3, 63, 64, 65, 200}, P in {2, 3, 7, 64}, n_gh in
{1, 20, 64} (at n_gh = 64 the tail weights underflow to 0), every matrix at a leading dimension larger than its
width with NaN in all padding; grf_rows_sqsum_f64 at len in {1, 63, 64, 65, 130}, groups in {1, 3, 7} and the same n.

Rule (the project's usual one): the GPU's error against the mpmath truth <= max(10 x the restatement's own error,
floor), floor = 4 (P + n_gh) u |value| (tests/test_svgp_reference.py: P - 1 factors of one erf at no more than 2 ulp
and two roundings each, an n_gh-term sum; |value| the quantity's largest magnitude among the case's truth rows,
for ve the magnitude of log(epsilon / (P - 1))).  The truth costs P n_gh multiprecision erf evaluations a row, so
it is taken on the first, middle and last row of every n (the first and last where P n_gh > 1000) and on every
edge row; all rows are held to the fp64 restatement, which follows the library's order, within twice the floor.  grf_rows_sqsum_f64 has no
transcendental: it equals the restatement bit for bit, and the np.longdouble sum within len u sum t^2.

Also: padding and inputs untouched, a second call gives the same bits, the forward-only call's ve equals the fused
call's bit for bit, an out-of-range label gives a NaN row and leaves its neighbours' bits, the edge rows of the CPU
test (mu = +-50, var in {0, 1e-12, 1e3}, the label first and last).

The figures are printed; measured on an MI355X, worst over n, GPU error (restatement's error, floor), at P = 7,
n_gh = 20: ve 1.5e-15 (1.8e-15, 1.0e-13), dmu 3.3e-16 (3.8e-16, 2.4e-14), dvar 1.4e-16 (1.3e-16, 2.1e-14), ps 5.9e-17
(8.9e-17, 1.2e-14); at P = 64, n_gh = 64: ve 2.8e-16 (2.8e-16, 6.3e-13), dmu 6.7e-20 (6.7e-20, 4.9e-18), dvar 8.3e-20
(5.6e-20, 9.4e-18), ps 3.3e-17 (4.7e-17, 5.7e-14).  Over all rows the GPU and the restatement differ by at most 2.7e-15;
on the edge rows by at most 8.9e-16.  rows_sqsum: the restatement's bits everywhere, worst error 0.79 of its bound.
DESIGN.md section 18 has the table.
"""
import functools

import numpy as np
import pytest

import svgp_reference as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 63, 64, 65, 200)
U = float(R.U)


@functools.lru_cache(maxsize=None)
def _pool(P):
    return R.random_rows(max(NS), P, 1000 + P)


@functools.lru_cache(maxsize=None)
def _gh(n_gh):
    return R.hermgauss(n_gh)


@functools.lru_cache(maxsize=None)
def _truth_row(P, n_gh, k):
    mu, var, y = _pool(P)
    gh_x, gh_w = _gh(n_gh)
    return R.ve_truth(mu[k], var[k], int(y[k]), gh_x, gh_w)


@functools.lru_cache(maxsize=None)
def _restated(P, n_gh):
    mu, var, y = _pool(P)
    gh_x, gh_w = _gh(n_gh)
    return R.variational_expectations(mu, var, y, gh_x, gh_w)


@pytest.fixture(scope="module")
def dev():
    import torch
    from grf_amd.engine import GRFEngine, _p
    eng = GRFEngine("cuda:0")
    return dict(torch=torch, eng=eng, p=_p)


def _padded(torch, a, ld):
    """An n x ld device matrix of NaN holding ``a`` in its first columns."""
    a = np.asarray(a, np.float64)
    t = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return t


def _ve_call(dev, mu, var, y, gh_x, gh_w, P, grad=True, epsilon=R.EPSILON, lds=(3, 1, 2, 5)):
    """One call on padded copies: (ve, dmu, dvar) as numpy bodies; asserts padding and inputs untouched."""
    torch, eng, p = dev["torch"], dev["eng"], dev["p"]
    from grf_amd import _lib
    n = mu.shape[0]
    tm, tv = _padded(torch, mu, P + lds[0]), _padded(torch, var, P + lds[1])
    ty = torch.from_numpy(np.asarray(y, np.int32)).cuda()
    gx, gw = torch.from_numpy(gh_x).cuda(), torch.from_numpy(gh_w).cuda()
    keep = [t.clone() for t in (tm, tv, ty, gx, gw)]
    ve = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    dm = torch.full((n, P + lds[2]), float("nan"), dtype=torch.float64, device="cuda") if grad else None
    dv = torch.full((n, P + lds[3]), float("nan"), dtype=torch.float64, device="cuda") if grad else None
    _lib.check(eng.lib.grf_robustmax_ve_f64(n, P, p(tm), P + lds[0], p(tv), P + lds[1], p(ty), p(gx), p(gw),
                                            len(gh_x), epsilon, p(ve), p(dm), P + lds[2], p(dv), P + lds[3],
                                            eng.stream), "grf_robustmax_ve_f64")
    torch.cuda.synchronize()
    for a, b in zip((tm, tv, gx, gw), keep[:2] + keep[3:]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "an input changed"
    assert torch.equal(ty, keep[2])
    if grad:
        assert bool(torch.isnan(dm[:, P:]).all()) and bool(torch.isnan(dv[:, P:]).all()), "padding written"
        return ve.cpu().numpy(), dm[:, :P].cpu().numpy(), dv[:, :P].cpu().numpy()
    return ve.cpu().numpy(), None, None


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _held(name, got, rest, truth, floor):
    """GPU error against the truth <= max(10 x restatement error, floor); (gpu error, restatement error)."""
    err = max(abs(R.mp(g) - t) for g, t in zip(np.ravel(got), truth))
    own = max(abs(R.mp(g) - t) for g, t in zip(np.ravel(rest), truth))
    assert err <= max(10 * own, floor), (name, float(err), float(own), floor)
    return float(err), float(own)


@pytest.mark.parametrize("n_gh", [1, 20, 64])
@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_variational_expectations_and_gradients(dev, P, n_gh):
    mu, var, y = _pool(P)
    gh_x, gh_w = _gh(n_gh)
    rve, rdmu, rdvar = _restated(P, n_gh)
    log_miss = abs(np.log(R.EPSILON / (P - 1)))
    worst = {}
    for n in NS:
        ve, dmu, dvar = _ve_call(dev, mu[:n], var[:n], y[:n], gh_x, gh_w, P)
        assert np.all(np.isfinite(ve)) and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
        ve2, dmu2, dvar2 = _ve_call(dev, mu[:n], var[:n], y[:n], gh_x, gh_w, P)
        assert _same_bits(ve, ve2) and _same_bits(dmu, dmu2) and _same_bits(dvar, dvar2), "a second call differs"
        ve3, _, _ = _ve_call(dev, mu[:n], var[:n], y[:n], gh_x, gh_w, P, grad=False)
        assert _same_bits(ve, ve3), "the forward-only call's ve differs from the fused call's"
        rows = sorted({0, n // 2, n - 1}) if P * n_gh <= 1000 else sorted({0, n - 1})
        truths = [_truth_row(P, n_gh, k) for k in rows]
        for name, got, rest, pick, mag in (
                ("ve", ve, rve, lambda t: [t[0]], log_miss),
                ("dmu", dmu, rdmu, lambda t: t[1], None), ("dvar", dvar, rdvar, lambda t: t[2], None)):
            truth = [v for t in truths for v in pick(t)]
            mag = mag if mag is not None else float(max(abs(v) for v in truth))
            floor = R.floor_p(P, n_gh, mag)
            err, own = _held(name, got[rows], rest[rows], truth, floor)
            # every row against the restatement (the library's order): both sit within the floor of the truth
            scale = mag if name == "ve" else max(np.abs(rest[:n]).max(), mag)
            diff = np.abs(got - rest[:n]).max()
            assert diff <= 2 * R.floor_p(P, n_gh, scale), (name, n, diff)
            w = worst.setdefault(name, [0.0, 0.0, 0.0, 0.0])
            worst[name] = [max(w[0], err), max(w[1], own), max(w[2], floor), max(w[3], diff)]
    for name, (err, own, floor, diff) in worst.items():
        print(f"P={P} n_gh={n_gh} {name}: gpu error {err:.3e}, restatement error {own:.3e}, floor {floor:.3e}, "
              f"max |gpu - restatement| over all rows {diff:.3e}")


@pytest.mark.parametrize("n_gh", [1, 20, 64])
@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_predictive_probabilities(dev, P, n_gh):
    torch, eng, p = dev["torch"], dev["eng"], dev["p"]
    from grf_amd import _lib
    mu, var, _ = _pool(P)
    gh_x, gh_w = _gh(n_gh)
    rest = R.predict_probabilities(mu, var, gh_x, gh_w)
    gx, gw = torch.from_numpy(gh_x).cuda(), torch.from_numpy(gh_w).cuda()
    floor = R.floor_p(P, n_gh, 1.0)
    classes = list(range(P)) if P * P * n_gh <= 4000 else [0, P // 2, P - 1]
    truth = []
    for c in classes:
        pc = R.prob_truth(mu[0], var[0], c, gh_x, gh_w)
        truth.append(pc * (1 - R.mp(R.EPSILON)) + (1 - pc) * R.mp(R.EPSILON) / (P - 1))
    worst = [0.0, 0.0, 0.0]
    for n in NS:
        tm, tv = _padded(torch, mu[:n], P + 2), _padded(torch, var[:n], P + 4)
        keep = (tm.clone(), tv.clone())
        outs = []
        for _ in range(2):
            ps = torch.full((n, P + 3), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(eng.lib.grf_robustmax_predict_f64(n, P, p(tm), P + 2, p(tv), P + 4, p(gx), p(gw), n_gh,
                                                         R.EPSILON, p(ps), P + 3, eng.stream),
                       "grf_robustmax_predict_f64")
            torch.cuda.synchronize()
            assert bool(torch.isnan(ps[:, P:]).all()), "padding written"
            outs.append(ps[:, :P].cpu().numpy())
        assert _same_bits(outs[0], outs[1]), "a second call differs"
        assert torch.equal(tm.view(torch.int64), keep[0].view(torch.int64))
        assert torch.equal(tv.view(torch.int64), keep[1].view(torch.int64))
        got = outs[0]
        assert np.all(np.isfinite(got)) and got.min() > 0.0 and got.max() < 1.0
        err, own = _held("ps", got[0, classes], rest[0, classes], truth, floor)
        diff = np.abs(got - rest[:n]).max()
        assert diff <= 2 * floor, (n, diff)
        worst = [max(worst[0], err), max(worst[1], own), max(worst[2], diff)]
    print(f"P={P} n_gh={n_gh} ps: gpu error {worst[0]:.3e}, restatement error {worst[1]:.3e}, floor {floor:.3e}, "
          f"max |gpu - restatement| over all rows {worst[2]:.3e}")


@pytest.mark.parametrize("n_gh", [1, 20])
@pytest.mark.parametrize("P", [2, 3, 7, 64])
def test_edge_rows(dev, P, n_gh):
    gh_x, gh_w = _gh(n_gh)
    mu, var, y = R.edge_rows(P)
    ve, dmu, dvar = _ve_call(dev, mu, var, y, gh_x, gh_w, P)
    rve, rdmu, rdvar = R.variational_expectations(mu, var, y, gh_x, gh_w)
    assert np.all(np.isfinite(ve)) and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    clipped = var < R.CLIP
    assert clipped.any() and np.all(dvar[clipped] == 0.0), "a clipped variance gets gradient 0"
    log_miss = abs(np.log(R.EPSILON / (P - 1)))
    for k in range(len(y)):                       # every edge row against the mpmath truth
        tve, tdmu, tdvar = R.ve_truth(mu[k], var[k], int(y[k]), gh_x, gh_w)
        _held("ve", ve[k:k + 1], rve[k:k + 1], [tve], R.floor_p(P, n_gh, log_miss))
        # per row: the rows' gradients span twenty orders of magnitude (var from 1e-10 to 1e3)
        for name, got, rest, truth in (("dmu", dmu[k], rdmu[k], tdmu), ("dvar", dvar[k], rdvar[k], tdvar)):
            mag = float(max(abs(v) for v in truth))
            _held(name, got, rest, truth, R.floor_p(P, n_gh, mag))
    # ... and against the restatement (the library's order), as in the main test: within twice the floor
    for name, got, rest, mag in (("ve", ve, rve, log_miss), ("dmu", dmu, rdmu, np.abs(rdmu).max()),
                                 ("dvar", dvar, rdvar, np.abs(rdvar).max())):
        assert np.abs(got - rest).max() <= 2 * R.floor_p(P, n_gh, mag), name
    print(f"P={P} n_gh={n_gh} edge rows: max |gpu - restatement| ve {np.abs(ve - rve).max():.3e}, "
          f"dmu {np.abs(dmu - rdmu).max():.3e}, dvar {np.abs(dvar - rdvar).max():.3e}")


def test_out_of_range_labels_give_nan_rows_and_leave_their_neighbours(dev):
    P, n_gh, n = 7, 20, 65
    mu, var, y = _pool(P)
    gh_x, gh_w = _gh(n_gh)
    good = _ve_call(dev, mu[:n], var[:n], y[:n], gh_x, gh_w, P)
    bad_y = y[:n].copy()
    bad = {3: -1, 10: np.iinfo(np.int32).max, 31: np.iinfo(np.int32).min, 64: P}
    for k, v in bad.items():
        bad_y[k] = v
    got = _ve_call(dev, mu[:n], var[:n], bad_y, gh_x, gh_w, P)
    fwd = _ve_call(dev, mu[:n], var[:n], bad_y, gh_x, gh_w, P, grad=False)
    ok = np.array([k not in bad for k in range(n)])
    for g, w in zip(got, good):
        assert np.all(np.isnan(g[~ok])), "an out-of-range label's row is not NaN"
        assert _same_bits(g[ok], w[ok]), "a neighbour of an out-of-range label changed"
    assert np.all(np.isnan(fwd[0][~ok])) and _same_bits(fwd[0][ok], good[0][ok])


@pytest.mark.parametrize("groups", [1, 3, 7])
def test_rows_sqsum(dev, groups):
    torch, eng, p = dev["torch"], dev["eng"], dev["p"]
    from grf_amd import _lib
    r = np.random.default_rng(50 + groups)
    worst = 0.0
    for length in (1, 63, 64, 65, 130):
        width = groups * length
        Tfull = r.standard_normal((max(NS), width)) * np.exp(r.standard_normal((max(NS), width)))
        bfull = r.standard_normal(max(NS))
        for n in NS:
            T, base = Tfull[:n], bfull[:n]
            tT = _padded(torch, T, width + 3)
            tb = torch.from_numpy(base).cuda()
            keep = tT.clone()
            for use_base in (True, False):
                outs = []
                for _ in range(2):
                    out = torch.full((n, groups + 2), float("nan"), dtype=torch.float64, device="cuda")
                    _lib.check(eng.lib.grf_rows_sqsum_f64(n, groups, length, p(tT), width + 3,
                                                          p(tb if use_base else None), p(out), groups + 2,
                                                          eng.stream), "grf_rows_sqsum_f64")
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(out[:, groups:]).all()), "padding written"
                    outs.append(out[:, :groups].cpu().numpy())
                assert _same_bits(outs[0], outs[1]), "a second call differs"
                rest = R.rows_sqsum(T, groups, base if use_base else None)
                assert _same_bits(outs[0], rest), (length, n, use_base, "the restatement's bits")
                sq = (T.astype(R.LD) ** 2).reshape(n, groups, length)
                truth = sq.sum(axis=2) + (base.astype(R.LD)[:, None] if use_base else 0)
                bound = (length + 1) * R.U * (sq.sum(axis=2) + (np.abs(base)[:, None] if use_base else 0))
                err = np.abs(outs[0].astype(R.LD) - truth)
                assert np.all(err <= bound), (length, n, use_base)
                worst = max(worst, float((err / np.maximum(bound, R.LD(1e-300))).max()))
            assert torch.equal(tT.view(torch.int64), keep.view(torch.int64)), "T changed"
    print(f"groups={groups}: bit-equal to the restatement; worst error / (len u sum t^2) {worst:.3e}")
    # len == 0 writes base (or 0); the engine's wrapper on a view with a larger pitch
    out = torch.full((3, groups), float("nan"), dtype=torch.float64, device="cuda")
    tb = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")
    _lib.check(eng.lib.grf_rows_sqsum_f64(3, groups, 0, None, 0, p(tb), p(out), groups, eng.stream), "len 0")
    assert torch.equal(out, tb[:, None].expand(3, groups))
    tT = _padded(torch, Tfull[:5], Tfull.shape[1] + 1)
    got = eng.rows_sqsum(tT[:, :Tfull.shape[1]], groups).cpu().numpy()
    assert _same_bits(got, R.rows_sqsum(Tfull[:5], groups))
