#!/usr/bin/env python3
"""Generate the item-item graph fixtures under tests/golden/{tiny,lastfm}/ by IMPORTING the reference's
preprocess_instacart_i2i.build_item_item (read-only reference tree) on the CPU, as make_golden.py does for the model.

TEST INFRASTRUCTURE ONLY: the outputs are data (indptr / indices / data of the reference's matrix and the wall-clock seconds
it took); nothing of the reference's source text is written to the repository.

Usage:  python tests/golden/make_golden_i2i.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_CODE = "/root/reference/LightGCN_work/code"

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
from i2i_restatement import FIXTURES, fixture_path      # noqa: E402


def main():
    sys.path.insert(0, REF_CODE)
    import preprocess_instacart_i2i as ref
    ref.tqdm = lambda it, **kw: it                       # no progress bars
    for name, weight, topk, min_basket in FIXTURES:
        train = os.path.join(HERE, name, "train.txt")
        n_items = ref.infer_n_items_from_files(train, os.path.join(HERE, name, "test.txt"))
        t0 = time.perf_counter()
        m = ref.build_item_item(train, n_items=n_items, topk=topk, weight=weight, min_basket=min_basket)
        sec = time.perf_counter() - t0
        m.sort_indices()
        out = fixture_path(HERE, name, weight, topk, min_basket)
        np.savez_compressed(out, indptr=m.indptr.astype(np.int32), indices=m.indices.astype(np.int32), data=m.data.astype(np.float32),
                            n_items=np.int64(n_items), seconds=np.float64(sec))
        print(f"{out}: nnz {m.nnz}, {sec:.3f} s, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
