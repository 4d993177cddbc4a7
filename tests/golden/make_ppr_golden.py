#!/usr/bin/env python3
"""Generate tests/golden/tiny/ppr_weights.npy by IMPORTING the reference's compute_ppr.compute_ppr_weights (read-only
reference tree) on the CPU, as make_golden.py does for the model: the [N, K+1] per-node layer weights of the `tiny`
fixture's bipartite user-item adjacency (binary, symmetric) for K = 3, alpha = 0.15 -- what --ppr_weights_path reads.

TEST INFRASTRUCTURE ONLY: the output is data (one fp32 array); nothing of the reference's source text is written to the
repository.

Usage:  python tests/golden/make_ppr_golden.py
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
REF_CODE = "/root/reference/LightGCN_work/code"
K, ALPHA = 3, 0.15

sys.dont_write_bytecode = True


def main():
    sys.path.insert(0, REF_CODE)
    import compute_ppr as ref
    z = np.load(os.path.join(HERE, "tiny", "golden.npz"))
    indptr, indices = z["adj_indptr"], z["adj_indices"]
    n = len(indptr) - 1
    adj = sp.csr_matrix((np.ones(len(indices), dtype=np.float64), indices, indptr), shape=(n, n)).tocoo()
    assert (abs(adj - adj.T)).nnz == 0
    w = np.asarray(ref.compute_ppr_weights(adj, alpha=ALPHA, K=K), dtype=np.float32)
    assert w.shape == (n, K + 1)
    out = os.path.join(HERE, "tiny", "ppr_weights.npy")
    np.save(out, w)
    print(f"{out}: shape {w.shape}, {os.path.getsize(out)} bytes, isolated nodes {int((np.diff(indptr) == 0).sum())}")


if __name__ == "__main__":
    main()
