"""CPU side of the item-item graph builder (ABI 13): the numpy restatement of its semantics (tests/i2i_restatement.py) against
the matrices recorded from the reference's own build_item_item (tests/golden/make_golden_i2i.py), the new flags, and the
argument checks of the binding that need no device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import i2i_restatement as R                     # noqa: E402
from conftest import GOLDEN                     # noqa: E402


@pytest.mark.parametrize("name,weight,topk,min_basket", R.FIXTURES, ids=lambda v: str(v))
def test_restatement_matches_reference_fixture(name, weight, topk, min_basket):
    """Structure exactly; values within (n_i + n_j + 16) 2^-24 |ref| (two fp32 summation orders of each row sum through sqrt,
    reciprocal and two multiplies, on both sides)."""
    z = np.load(R.fixture_path(GOLDEN, name, weight, topk, min_basket))
    indptr, indices = R.baskets_csr(R.read_baskets(os.path.join(GOLDEN, name, "train.txt")))
    m = R.build(indptr, indices, int(z["n_items"]), topk, weight, min_basket)
    assert m.indptr.dtype.kind == "i" and m.data.dtype == np.float32
    R.assert_csr_close(m, R.Csr(z["indptr"], z["indices"], z["data"]), f"{name} {weight} topk={topk} min_basket={min_basket}")
    assert float(z["seconds"]) > 0.0


def test_fixtures_are_small():
    for f in R.FIXTURES:
        assert os.path.getsize(R.fixture_path(GOLDEN, *f)) < (1 << 20), f


def test_tie_rule_on_a_hand_case():
    """All counts 1: the cut is decided by the first basket, then the column."""
    baskets = [np.array([3, 1]), np.array([0, 1, 2]), np.array([1, 4, 5])]
    indptr, indices = R.baskets_csr(baskets)
    r = R.Restatement(indptr, indices, 7)
    j, w, first = r.row(1, "cooc")
    assert j.tolist() == [3, 0, 2, 4, 5] and first.tolist() == [0, 1, 1, 2, 2] and w.tolist() == [1.0] * 5
    assert r.deg.tolist() == [1, 3, 1, 1, 1, 1, 0] and r.total == 3.0 and r.work[1] == 5
    r3 = R.Restatement(indptr, indices, 7, min_basket=3)
    assert r3.total == 2.0 and r3.row(1, "cooc")[0].tolist() == [0, 2, 4, 5] and r3.row(3, "cooc")[0].size == 0


def test_flags(pkg):
    w = pkg.world
    w.configure([])
    assert (w.config['i2i_build'], w.config['i2i_topk'], w.config['i2i_min_basket']) == ('none', 50, 1)
    w.configure(['--use_item_item', '--i2i_build', 'pmi', '--i2i_topk', '7', '--i2i_min_basket', '3'])
    assert (w.config['i2i_build'], w.config['i2i_topk'], w.config['i2i_min_basket']) == ('pmi', 7, 3)
    with pytest.raises(SystemExit):
        w.configure(['--i2i_build', 'cosine'])
    w.configure([])


def test_binding_declares_the_two_stages(pkg):
    assert pkg._lib.ABI_VERSION == 13
    assert {"lgcn_i2i_topk", "lgcn_i2i_finish"} <= set(pkg._lib.SIGNATURES)
    lib = pkg._lib.load()
    assert hasattr(lib, "lgcn_i2i_topk") and hasattr(lib, "lgcn_i2i_finish")
    assert pkg._lib.I2I_WEIGHTS == {"cooc": 0, "jaccard": 1, "pmi": 2}


def test_wrapper_value_errors_without_a_device(pkg):
    import torch
    L = pkg._lib
    ip = torch.tensor([0, 2, 3], dtype=torch.int64)
    ix = torch.tensor([0, 1, 1], dtype=torch.int32)
    for kw in ({"topk": 0}, {"topk": 257}, {"weight": "cosine"}, {"min_basket": -1}, {"m_items": 0}, {"m_items": -3},
               {"m_items": 2 ** 23, "topk": 256}):
        args = {"m_items": 4, "topk": 5, "weight": "cooc", "min_basket": 1}
        args.update(kw)
        with pytest.raises(ValueError):
            L.i2i_topk(ip, ix, **args)
    with pytest.raises(ValueError, match="device"):
        L.i2i_topk(ip, ix, 4)                                            # host tensors
    with pytest.raises(ValueError):
        L.i2i_topk(ip.to(torch.int32), ix, 4)
    with pytest.raises(ValueError):
        L.i2i_topk([0, 2, 3], ix, 4)
    cols = torch.full((4, 5), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match="device"):
        L.i2i_finish(cols, torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        L.i2i_finish(torch.zeros(4, dtype=torch.int32), torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))


def test_module_mirrors_the_reference_surface(pkg, tiny, tmp_path):
    m = pkg.preprocess_instacart_i2i
    train, test = os.path.join(tiny.dir, "train.txt"), os.path.join(tiny.dir, "test.txt")
    assert m.infer_n_items_from_files(train, test) == tiny.m_items
    assert m.infer_n_items_from_files(train, os.path.join(str(tmp_path), "missing.txt")) <= tiny.m_items
    with pytest.raises(ValueError, match="weight"):
        m.build_item_item(train, weight="cosine")                        # the reference would silently use cooc
    indptr, indices = m.read_baskets(train)
    ip, ix = R.baskets_csr(R.read_baskets(train))
    assert np.array_equal(indptr, ip) and np.array_equal(indices, ix)
    p = os.path.join(str(tmp_path), "odd.txt")
    with open(p, "w") as f:
        f.write("0 5 3 5 1\n7\n\n2 9\n")
    indptr, indices = m.read_baskets(p)
    assert indptr.tolist() == [0, 3, 4] and indices.tolist() == [1, 3, 5, 9]
    assert m.infer_n_items_from_files(p) == 10
    with pytest.raises(ValueError, match="item id"):
        m.build_from_csr(indptr, indices, 9)
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int64))
    for kw in ({"topk": 0}, {"topk": 257}, {"min_basket": -1}, {"weight": "cosine"}):      # checked before anything else, on empty data too
        for n in (0, 9):
            with pytest.raises(ValueError):
                m.build_from_csr(*empty, n, **kw)
    assert m.build_from_csr(*empty, 0).shape == (0, 0)
    assert m.infer_n_items_from_files(os.path.join(str(tmp_path), "missing.txt")) == 0
    import torch
    if not torch.cuda.is_available():                                    # no CPU fallback
        with pytest.raises(pkg._lib.LgcnError):
            m.build_item_item(train, topk=5)
