"""Generate tests/golden/expm.npz by running the *reference's* diffusion_kernel
(efficient_graph_gp/graph_kernels/diffusion_kernel.py:6-12: scipy.linalg.expm of -beta times the normalised
Laplacian of graph_kernels/utils.py:22-26).

Run once where a checkout of the reference is available:
    python tests/golden/make_expm_golden.py <path to the reference checkout>
The output is data only (adjacency matrices and the expected exp(-beta L)); nothing of the reference's source
is stored.  Two graphs: the 4-node toy of the reference's README, and a seeded 40-node graph with one isolated
node (whose Laplacian row the reference leaves as e_i); beta in {0.5, 2}.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
BETAS = (0.5, 2.0)


def graphs():
    toy = np.array([[0, 1, 1, 0], [1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 0]], dtype=np.float64)
    rng = np.random.default_rng(40)
    n = 40
    W = np.triu((rng.random((n, n)) < 0.15).astype(np.float64), 1)
    W = W + W.T
    W[7, :] = 0.0
    W[:, 7] = 0.0
    return {"toy": toy, "isolated": W}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from efficient_graph_gp.graph_kernels.diffusion_kernel import diffusion_kernel

    out = {"betas": np.asarray(BETAS)}
    for name, W in graphs().items():
        out[name + "_adj"] = W
        for beta in BETAS:
            out[f"{name}_K_{beta:g}"] = np.asarray(diffusion_kernel(W, beta=beta), dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "expm.npz"), **out)


if __name__ == "__main__":
    main()
