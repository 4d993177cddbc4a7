"""numpy restatement of the item-item builder's semantics (preprocess_instacart_i2i.py:61-170 of the reference), row by row:
test infrastructure for tests/test_i2i_restatement.py (which pins it to the reference's recorded outputs) and
tests/test_gpu_i2i.py (which compares the HIP kernels with it).  Each row comes from its baskets directly.

Order of a row's neighbours: weight descending, then the first kept basket holding both items ascending, then j ascending --
what heapq.nlargest (stable) makes of a dict filled by combinations(sorted(items), 2) basket after basket."""
import math

import numpy as np
import scipy.sparse as sp

EPS32 = 2.0 ** -24
WEIGHTS = ("cooc", "jaccard", "pmi")


def read_baskets(path):
    """The reference's reading rule: line order, lines with fewer than two fields skipped, each line's items deduplicated."""
    out = []
    with open(path) as f:
        for line in f:
            parts = line.strip().split()
            if len(parts) < 2:
                continue
            out.append(np.unique(np.asarray([int(x) for x in parts[1:]], np.int64)))
    return out


def baskets_csr(baskets):
    sizes = np.asarray([len(b) for b in baskets], np.int64)
    indptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    indices = (np.concatenate(baskets) if len(baskets) else np.zeros(0)).astype(np.int32)
    return indptr, indices


class Restatement:
    def __init__(self, indptr, indices, n_items, min_basket=1):
        self.indptr = np.asarray(indptr, np.int64)
        self.indices = np.asarray(indices, np.int64)
        self.n_items = int(n_items)
        self.sizes = np.diff(self.indptr)
        nb = len(self.sizes)
        kept = self.sizes >= min_basket
        n_kept = int(kept.sum())
        self.total = float(n_kept) if n_kept > 0 else 1.0
        bid = np.repeat(np.arange(nb, dtype=np.int64), self.sizes)
        m = kept[bid]
        it, bb = self.indices[m], bid[m]
        self.deg = np.bincount(it, minlength=self.n_items).astype(np.int64)
        order = np.argsort(it, kind="stable")
        self.t_b = bb[order]
        self.t_ptr = np.concatenate([[0], np.cumsum(self.deg)])
        self.work = np.zeros(self.n_items, np.int64)                 # sum over the item's kept baskets of |b| - 1
        np.add.at(self.work, it, (self.sizes[bb] - 1))

    def row(self, i, weight):
        """All neighbours of item i, best first: (j int64, w float64, first basket int64)."""
        bs = self.t_b[self.t_ptr[i]:self.t_ptr[i + 1]]
        if len(bs) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)
        lens = self.sizes[bs]
        off = np.repeat(self.indptr[bs] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
        items, bb = self.indices[off], np.repeat(bs, lens)
        m = items != i
        items, bb = items[m], bb[m]
        if len(items) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)
        j, inv, c = np.unique(items, return_inverse=True, return_counts=True)
        first = np.full(len(j), np.iinfo(np.int64).max)
        np.minimum.at(first, inv, bb)
        di, dj = int(self.deg[i]), self.deg[j]
        if weight == "cooc":
            w = c.astype(np.float64)
        elif weight == "jaccard":
            den = di + dj - c
            w = np.where(den <= 0, 0.0, c.astype(np.float64) / np.where(den <= 0, 1, den).astype(np.float64))
        elif weight == "pmi":
            total = self.total
            w = np.asarray([max(math.log((float(cc) * total) / (float(di) * float(d)) + 1e-12), 0.0) if di * d > 0 else 0.0
                            for cc, d in zip(c.tolist(), dj.tolist())], np.float64)
        else:
            raise ValueError(weight)
        order = np.lexsort((j, first, -w))
        return j[order], w[order], first[order]

    def lists(self, weight, topk, items=None):
        """{i: (cols, w64)} of the topk best, in rank order, for the given items (default: all)."""
        out = {}
        for i in (range(self.n_items) if items is None else items):
            j, w, _ = self.row(int(i), weight)
            out[int(i)] = (j[:topk], w[:topk])
        return out


def finish(rows, cols, w32, n_items):
    """Symmetrise by maximum and normalise, with scipy, as the reference does (:152-170)."""
    a = sp.csr_matrix((np.asarray(w32, np.float32), (np.asarray(rows, np.int64), np.asarray(cols, np.int64))),
                      shape=(n_items, n_items), dtype=np.float32)
    a = a.maximum(a.transpose())
    deg = np.ravel(a.sum(axis=1)).astype(np.float32)
    deg[deg == 0.0] = 1.0
    inv = 1.0 / np.sqrt(deg)
    a = a.multiply(inv[:, None]).multiply(inv[None, :]).tocsr()
    a.sort_indices()
    return a


def build(indptr, indices, n_items, topk, weight, min_basket=1):
    r = Restatement(indptr, indices, n_items, min_basket)
    rows, cols, vals = [], [], []
    for i, (j, w) in r.lists(weight, topk).items():
        rows.append(np.full(len(j), i, np.int64)); cols.append(j); vals.append(w.astype(np.float32))
    return finish(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n_items)


def value_bound(indptr, indices, ref):
    """(n_i + n_j + 16) 2^-24 |ref| per entry: the first-order bound on two fp32 summation orders of each row sum, through the
    square root, the reciprocal and the two multiplies, on both sides."""
    n = np.diff(np.asarray(indptr, np.int64))
    rows = np.repeat(np.arange(len(n)), n)
    return (n[rows] + n[np.asarray(indices, np.int64)] + 16) * EPS32 * np.abs(np.asarray(ref, np.float64))


def assert_csr_close(got, ref, what=""):
    """Structure exactly, values within value_bound.  got / ref: anything with indptr, indices, data."""
    gp, gi, gd = np.asarray(got.indptr, np.int64), np.asarray(got.indices, np.int64), np.asarray(got.data)
    rp, ri, rd = np.asarray(ref.indptr, np.int64), np.asarray(ref.indices, np.int64), np.asarray(ref.data)
    assert gp.shape == rp.shape and np.array_equal(gp, rp), (what, "indptr")
    assert np.array_equal(gi, ri), (what, "indices")
    err = np.abs(gd.astype(np.float64) - rd.astype(np.float64))
    bound = value_bound(rp, ri, rd)
    bad = err > bound
    print(f"[i2i] {what}: nnz {len(rd)}, max |err| {err.max() if len(err) else 0.0:.3e}, max err/bound "
          f"{(err / np.maximum(bound, 1e-300)).max() if len(err) else 0.0:.3f}")
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()))


class Csr:
    def __init__(self, indptr, indices, data):
        self.indptr, self.indices, self.data = indptr, indices, data


def fixture_path(golden_dir, name, weight, topk, min_basket=1):
    import os
    tag = f"i2i_{weight}_k{topk}" + (f"_mb{min_basket}" if min_basket != 1 else "")
    return os.path.join(golden_dir, name, tag + ".npz")


FIXTURES = ([("tiny", w, k, 1) for w in WEIGHTS for k in (5, 50)] + [("tiny", "jaccard", 5, 3)] +
            [("lastfm", w, k, 1) for w in WEIGHTS for k in (5, 20)])
