"""Device-less harness for the C ABI's argument and capacity contracts.

An entry point of include/grf.h checks its arguments on the host before anything touches a device, so the checks
can be exercised with made-up pointers that are never dereferenced -- as long as every check is there.  A check
that went missing would turn such a call into a launch on made-up addresses, so the one rule of this module is:

    no made-up pointer is handed to an entry point in a process that can see a GPU.

`device_less_lib()` returns the loaded library itself when `grf_device_count() == 0`.  Otherwise it returns a
proxy with the library's call surface (`lib.grf_x(...)`, `lib.grf_last_error()`): every call is sent to one fresh
child process started with ROCR_VISIBLE_DEVICES and HIP_VISIBLE_DEVICES empty, which refuses to serve unless its
own `grf_device_count()` is 0; the parent only reads the child's answers.  Without a device an unguarded call
reaches a HIP call and comes back GRF_EHIP ("no ROCm-capable device is detected"); a guarded one comes back
GRF_EINVAL, GRF_EUNSUPPORTED or GRF_ECAPACITY.  Guard presence is thereby testable with no GPU.

Tables state one case as `Case(entry, args, status, substr)`; `run_cases` executes them and `failures` lists the
cases whose status or grf_last_error() differ.
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OK, EINVAL, EHIP, ECAPACITY, EUNSUPPORTED = 0, -1, -2, -3, -4
STATUS_NAMES = {OK: "GRF_OK", EINVAL: "GRF_EINVAL", EHIP: "GRF_EHIP", ECAPACITY: "GRF_ECAPACITY",
                EUNSUPPORTED: "GRF_EUNSUPPORTED"}


def P(k: int, off: int = 0) -> int:
    """Made-up device pointer number k (16 MiB apart, 256-byte aligned, never dereferenced) plus a byte offset."""
    return (k << 24) + off


# ------------------------------------------------------------------ argument encoding
# A call's arguments travel to the child as JSON: integers, floats (NaN and inf included), None, and
# {"host": hex} for host memory the entry reads itself (the walk parameter struct, the arrays of per-step device
# pointers), rebuilt in the child as a buffer of the same bytes.

def _encode(a):
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, dict) and set(a) == {"host"}:            # (host_ptrs / walk_params: encoded already)
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_double)):
        return a.value
    if hasattr(a, "_obj"):                                    # ctypes.byref(x)
        a = a._obj
    elif isinstance(a, ctypes._Pointer):                      # ctypes.pointer(x)
        a = a.contents
    if isinstance(a, (ctypes.Structure, ctypes.Array)):
        return {"host": bytes(a).hex()}
    raise TypeError(f"abi_contract: cannot send {type(a).__name__} to the device-less child")


def _decode(a, keep):
    if isinstance(a, dict):
        buf = ctypes.create_string_buffer(bytes.fromhex(a["host"]), max(len(a["host"]) // 2, 1))
        keep.append(buf)
        return ctypes.cast(buf, ctypes.c_void_p)
    return a


def host_ptrs(*ptrs) -> dict:
    """A host array of device pointers (grf_phi_steps_csr_*'s step_ptr / step_idx / step_val)."""
    return _encode((ctypes.c_void_p * len(ptrs))(*ptrs))


def walk_params(m=8, p=0.1, L=4, load_rule=0, rng=1, n_chunks=1, seed=42) -> dict:
    from grf_amd import _lib
    return _encode(_lib.GrfWalkParams(m, p, L, load_rule, rng, 0, n_chunks, seed))


def _call(lib, name, args):
    from grf_amd import _lib
    keep = []
    real = [_decode(a, keep) for a in args]
    argtypes = _lib.SIGNATURES[name][1]
    for i, (a, t) in enumerate(zip(real, argtypes)):
        if isinstance(a, ctypes.c_void_p) and t is not ctypes.c_void_p:   # POINTER(GrfWalkParams)
            real[i] = ctypes.cast(a, t)
    out = getattr(lib, name)(*real)
    return out


# ------------------------------------------------------------------ the child
def _serve() -> int:
    from grf_amd import _lib
    lib = _lib.load()
    seen = int(lib.grf_device_count())
    sys.stdout.write(json.dumps({"devices": seen}) + "\n")
    sys.stdout.flush()
    if seen != 0:                                             # (never call with made-up pointers beside a GPU)
        return 3
    for line in sys.stdin:
        req = json.loads(line)
        out = _call(lib, req["fn"], req["args"])
        if isinstance(out, bytes):
            out = {"bytes": out.decode("latin-1")}
        sys.stdout.write(json.dumps({"out": out}) + "\n")
        sys.stdout.flush()
    return 0


class _ChildLib:
    """The library's call surface, served by the device-less child."""

    def __init__(self):
        env = dict(os.environ)
        env["ROCR_VISIBLE_DEVICES"] = ""
        env["HIP_VISIBLE_DEVICES"] = ""
        self._proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], env=env,
                                      stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        atexit.register(self.close)
        hello = self._proc.stdout.readline()
        while hello and not hello.startswith("{"):            # (a library's own chatter before the first answer)
            hello = self._proc.stdout.readline()
        seen = json.loads(hello)["devices"] if hello.strip() else None
        if seen != 0:
            self.close()
            raise RuntimeError(f"abi_contract: the child started without visible devices still sees {seen}; "
                               "refusing to call entry points with made-up pointers")

    def close(self):
        proc, self._proc = self._proc, None
        if proc is not None:
            try:
                proc.stdin.close()
                proc.wait(timeout=30)
            except Exception:
                proc.kill()
                proc.wait()

    def __getattr__(self, name):
        if not name.startswith("grf_"):
            raise AttributeError(name)

        def fn(*args):
            self._proc.stdin.write(json.dumps({"fn": name, "args": [_encode(a) for a in args]}) + "\n")
            self._proc.stdin.flush()
            line = self._proc.stdout.readline()
            while line and not line.startswith('{"out"'):
                line = self._proc.stdout.readline()
            if not line.strip():
                raise RuntimeError(f"abi_contract: the device-less child died in {name}")
            out = json.loads(line)["out"]
            return out["bytes"].encode("latin-1") if isinstance(out, dict) else out
        return fn


class _LocalLib:
    """The loaded library behind the same argument encoding (no device visible in this process)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if not name.startswith("grf_"):
            raise AttributeError(name)
        return lambda *args: _call(self._lib, name, [_encode(a) for a in args])


_device_less = None


def device_less_lib():
    """The library for calls with made-up pointers: in-process only where no device is visible."""
    global _device_less
    if _device_less is None:
        from grf_amd import _lib
        lib = _lib.load()
        _device_less = _LocalLib(lib) if int(lib.grf_device_count()) == 0 else _ChildLib()
    return _device_less


# ------------------------------------------------------------------ tables
Case = collections.namedtuple("Case", "entry args status substr")


def run_cases(cases):
    """[(status, grf_last_error())] of the cases, each after a refusal of another entry, so that a message
    found afterwards is the case's own."""
    lib = device_less_lib()
    out = []
    for c in cases:
        primer = "grf_gram_mirror" if c.entry != "grf_gram_mirror" else "grf_hub_panel"
        if primer == "grf_gram_mirror":
            assert lib.grf_gram_mirror(-1, None, 0, 0, None) == EINVAL
        else:
            assert lib.grf_hub_panel(-1, None, None, None, None, None, 0, None) == EINVAL
        before = lib.grf_last_error()
        rc = getattr(lib, c.entry)(*c.args)
        err = lib.grf_last_error()
        out.append((rc, b"" if err == before else err))
    return out


def failures(cases):
    """The cases that did not come back as stated, as readable lines (empty: the table holds)."""
    bad = []
    for c, (rc, err) in zip(cases, run_cases(cases)):
        want = c.status if isinstance(c.status, tuple) else (c.status,)
        if rc not in want:
            bad.append(f"{c.entry}{tuple(c.args)}: {STATUS_NAMES.get(rc, rc)} ({err.decode(errors='replace')!r}), "
                       f"expected {' or '.join(STATUS_NAMES[w] for w in want)}")
        elif rc != OK and (not err or c.substr.encode() not in err):
            bad.append(f"{c.entry}{tuple(c.args)}: {STATUS_NAMES[rc]} with message {err.decode(errors='replace')!r}, "
                       f"expected one holding {c.substr!r} set by this call")
    return bad


if __name__ == "__main__":
    sys.exit(_serve() if sys.argv[1:] == ["--serve"] else 2)
