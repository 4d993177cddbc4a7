"""Item-item adjacency builder, mirror of the reference's preprocess_instacart_i2i.py (same names, arguments and CLI flags),
computed on the GPU: lgcn_i2i_topk + lgcn_i2i_finish (include/lgcn_hip.h) instead of the reference's
dict-of-dicts loop over every pair of every basket (:86-108), its per-row heapq.nlargest (:136-150) and scipy's
maximum / multiply (:161-168).

    python -m graph-and-sequential-recommendation-systems_amd.preprocess_instacart_i2i --data_root data/instacart --topk 50 --weight jaccard

The one deliberate difference: an unknown `weight` raises ValueError (the reference treats it as 'cooc' without a word).
There is no CPU fallback, like the rest of the package."""
import argparse
import os

import numpy as np

from . import _lib


def _item_lines(path):
    """The item ids of every usable line of an interaction file (`user item item ...`), as int64 arrays in file order.  A line that
    names no item is not a basket and is passed over; a path that is None or does not exist yields nothing."""
    if not path or not os.path.isfile(path):
        return
    with open(path) as fh:
        for raw in fh:
            fields = raw.split()
            if len(fields) >= 2:
                yield np.asarray(fields[1:], dtype=np.int64)


def infer_n_items_from_files(train_path, test_path=None):
    """Size of the item vocabulary: one more than the largest item id either file names (0 when they name none)."""
    top = [int(ids.max()) for path in (train_path, test_path) for ids in _item_lines(path)]
    return max(top) + 1 if top else 0


def read_baskets(train_path):
    """train.txt -> the baskets as a host CSR (indptr int64, indices int64): one basket per usable line, in file order, every
    basket's items made distinct (ascending)."""
    baskets = [np.unique(ids) for ids in _item_lines(train_path)]
    indptr = np.zeros(len(baskets) + 1, np.int64)
    np.cumsum([len(b) for b in baskets], out=indptr[1:])
    indices = np.concatenate(baskets) if baskets else np.zeros(0, np.int64)
    return indptr, indices


def build_from_csr(indptr, indices, n_items, topk=50, weight="cooc", min_basket=1, device=None):
    """Baskets as a host CSR (items distinct within a row, any order) -> the degree-normalised symmetric item-item graph,
    scipy.sparse.csr_matrix fp32 [n_items, n_items] with sorted columns.  Both stages run on the GPU."""
    import scipy.sparse as sp
    import torch
    if weight not in _lib.I2I_WEIGHTS:
        raise ValueError(f"weight must be one of {sorted(_lib.I2I_WEIGHTS)}, got {weight!r}")
    if int(min_basket) < 0:
        raise ValueError(f"min_basket={min_basket} must be >= 0")
    n_items = int(n_items)
    if n_items <= 0:                                           # no vocabulary at all: topk is still checked
        _lib._i2i_sizes(1, topk)
        if np.size(indices):
            raise ValueError(f"item id outside [0, n_items={n_items})")
        return sp.csr_matrix((0, 0), dtype=np.float32)
    n_items, topk = _lib._i2i_sizes(n_items, topk)
    indptr = np.ascontiguousarray(indptr, np.int64)
    indices = np.ascontiguousarray(indices)
    if indices.size and (int(indices.min()) < 0 or int(indices.max()) >= n_items):
        raise ValueError(f"item id outside [0, n_items={n_items})")
    _lib.require_gpu()
    if indices.size == 0:                                      # no basket: nothing co-occurs, every row is empty
        return sp.csr_matrix((n_items, n_items), dtype=np.float32)
    dev = torch.device(device if device is not None else "cuda")
    cols, w, length = _lib.i2i_topk(torch.from_numpy(indptr).to(dev), torch.from_numpy(indices.astype(np.int32)).to(dev),
                                    n_items, topk, weight, min_basket)
    ip, ix, vals, nnz = _lib.i2i_finish(cols, w, length)
    m = sp.csr_matrix((vals[:nnz].cpu().numpy(), ix[:nnz].cpu().numpy(), ip.cpu().numpy()), shape=(n_items, n_items), dtype=np.float32)
    m.has_sorted_indices = True
    return m


def build_item_item(train_path, n_items=None, topk=50, weight="cooc", min_basket=1):
    """The reference's entry point, same arguments: train.txt -> scipy.sparse.csr_matrix, fp32, [n_items, n_items], columns sorted.
    n_items None = infer_n_items_from_files(train_path); topk in 1..256; weight 'cooc', 'jaccard' or 'pmi' (anything else is a
    ValueError); a basket with fewer than min_basket distinct items does not count."""
    if weight not in _lib.I2I_WEIGHTS:
        raise ValueError(f"weight must be one of {sorted(_lib.I2I_WEIGHTS)}, got {weight!r}")
    indptr, indices = read_baskets(train_path)
    if n_items is None:
        n_items = infer_n_items_from_files(train_path)
    return build_from_csr(indptr, indices, n_items, topk=topk, weight=weight, min_basket=min_basket)


# the reference's command line: flag, type, default (choices for --weight); same names, types and defaults
_FLAGS = (("--data_root", str, "../data/instacart"), ("--train_file", str, "train.txt"), ("--test_file", str, "test.txt"),
          ("--out", str, "i2i_adj.npz"), ("--topk", int, 50), ("--weight", str, "cooc"), ("--min_basket", int, 1),
          ("--n_items", int, None))


def main(argv=None):
    """Build the graph of <data_root>/<train_file> and write it, as scipy's save_npz does, to <data_root>/<out>.  Returns the path."""
    from scipy.sparse import save_npz
    parser = argparse.ArgumentParser(description="item-item graph of an interaction file, built on the GPU")
    for flag, kind, default in _FLAGS:
        parser.add_argument(flag, type=kind, default=default, **({"choices": sorted(_lib.I2I_WEIGHTS)} if flag == "--weight" else {}))
    a = parser.parse_args(argv)
    train = os.path.join(a.data_root, a.train_file)
    n_items = a.n_items if a.n_items else infer_n_items_from_files(train, os.path.join(a.data_root, a.test_file))
    graph = build_item_item(train, n_items=n_items, topk=a.topk, weight=a.weight, min_basket=a.min_basket)
    os.makedirs(a.data_root, exist_ok=True)
    target = os.path.join(a.data_root, a.out)
    save_npz(target, graph)
    print(f"[I2I] wrote {target}: {graph.shape[0]} items, {graph.nnz} entries ({a.weight}, topk {a.topk})")
    return target


if __name__ == "__main__":
    main()
