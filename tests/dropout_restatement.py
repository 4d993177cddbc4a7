"""Host restatement of the edge-dropout mask (DESIGN 4 "Edge dropout"): keep(i, j) = H(seed, step, i, j) < floor(p 2^32) with H a
hash of the adjacency's row and column ids only, and of the weights the kernels stage for the survivors (drop_apply of
csrc/lgcn_device.hip: fl32(val * fl32(1 / p)), exact in float64).  Test infrastructure: tests/test_gpu_dropout.py compares the
exported mask (lgcn_dropout_mask) with it, tests/test_storage_restatement.py and tests/test_gpu_storage_step.py build the dropped
graph and -- explicitly, the mask is not symmetric -- its transpose from it."""
import numpy as np


def _splitmix64(z):
    M = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _fmix32(h):
    h = h.astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & M
    h ^= h >> np.uint64(16)
    return h


def _keep_host(rows, cols, keep, seed, step):
    k = _splitmix64((_splitmix64(seed & ((1 << 64) - 1)) + step) & ((1 << 64) - 1))
    k0, k1 = np.uint64(k & 0xFFFFFFFF), np.uint64(k >> 32)
    i, j = rows.astype(np.uint64), cols.astype(np.uint64)
    h = _fmix32(_fmix32(i ^ k0) ^ ((j * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) ^ k1)
    return h < np.uint64(int(np.floor(float(np.float32(keep)) * 4294967296.0)))


def _rows_of(a):
    return np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))


def a_scaled(vals, keep):
    """the survivors' weights as the kernels stage them: fl32(val * fl32(1 / keep)) -- within 1 ulp of val / keep"""
    return (vals.astype(np.float32) * (np.float32(1.0) / np.float32(keep))).astype(np.float32)


def dropped_graphs(a, keep, seed, step):
    """(A_drop, the matrix the backward launches multiply by) of one step as scipy CSR with A's structure and fp32 values, the
    dropped entries stored as explicit zeros.  The backward's entry stored at (i, j) carries keep(j, i) and the weight stored at
    (i, j) (dr.tr = 1): A_drop^T exactly, as the stored weights are symmetric (asserted by the CPU tests).  keep >= 1: (A, A)."""
    import scipy.sparse as sp
    if not keep < 1.0:
        return a, a
    rows, cols = _rows_of(a), a.indices
    vals, zero = a_scaled(a.data, keep), np.float32(0)
    fwd = np.where(_keep_host(rows, cols, keep, seed, step), vals, zero).astype(np.float32)
    bwd = np.where(_keep_host(cols, rows, keep, seed, step), vals, zero).astype(np.float32)
    return tuple(sp.csr_matrix((v, a.indices.copy(), a.indptr.copy()), shape=a.shape) for v in (fwd, bwd))
