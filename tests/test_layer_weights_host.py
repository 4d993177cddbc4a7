"""Weighted layer combination (--layer_weights, --ppr_alpha, the reference's --use_ppr_weights / --ppr_weights_path): everything
that needs no device -- the ABI surface, the flags' way into the config, the resolver's values, the PPR file loader against a
fixture written by the reference's own compute_ppr_weights, and the refusals that must be raised before any device call."""
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, REPO

NEW_SYMBOLS = ("lgcn_ctx_set_layer_weights", "lgcn_ctx_get_layer_weights", "lgcn_propagate_weighted")


def test_new_symbols_in_header_binding_and_library(pkg):
    hdr = open(os.path.join(REPO, "include", "lgcn_hip.h")).read()
    assert int(re.search(r"#define\s+LGCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 13      # additive: the ABI stays 13
    assert pkg._lib.ABI_VERSION == 13
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    lib = pkg._lib.load()
    assert lib.lgcn_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    # the argument checks that need no device
    w = np.array([0.4, 0.3, 0.2, 0.1], np.float32)
    assert lib.lgcn_ctx_set_layer_weights(None, w.ctypes.data, 4) == 3
    assert lib.lgcn_ctx_get_layer_weights(None, None) == 0
    assert lib.lgcn_propagate_weighted(None, None, 3, 64, 0, None, w.ctypes.data, None, None) == 3
    assert lib.lgcn_propagate_weighted(None, None, 3, 64, 0, None, None, None, None) == 3
    assert b"layer weights" in lib.lgcn_last_error()


def test_flags_reach_the_config(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['layer_weights'] == 'mean' and w.config['ppr_alpha'] == 0.15
        assert w.config['use_ppr_weights'] is False and w.config['ppr_weights_path'] is None and w.config['exp_smooth_beta'] == 0.5
        w.configure(['--layer_weights', 'ppr', '--ppr_alpha', '0.2'])
        assert w.config['layer_weights'] == 'ppr' and w.config['ppr_alpha'] == 0.2
        w.configure(['--layer_weights', '[0.4,0.3,0.2,0.1]'])
        assert w.config['layer_weights'] == '[0.4,0.3,0.2,0.1]'
    finally:
        w.configure([])


def test_resolver_values(pkg):
    R = pkg.model.resolve_layer_weights
    assert R({}, 3) is None and R({'layer_weights': 'mean'}, 3) is None
    w = R({'layer_weights': 'exp', 'exp_smooth_beta': 0.5}, 3)
    assert w.dtype == np.float32 and np.array_equal(w, (np.array([8, 4, 2, 1], np.float64) / 15).astype(np.float32))
    assert np.array_equal(R({'layer_weights': 'exp'}, 3), w)                              # the reference's default beta
    a = 0.15
    v = a * (1 - a) ** np.arange(4, dtype=np.float64)
    p = R({'layer_weights': 'ppr', 'ppr_alpha': a}, 3)
    assert p.dtype == np.float32 and np.array_equal(p, (v / v.sum()).astype(np.float32)) and abs(float(p.sum()) - 1) < 1e-6
    assert np.array_equal(R({'layer_weights': 'ppr'}, 3), p)                              # compute_ppr.py's default alpha
    assert len(R({'layer_weights': 'ppr'}, 1)) == 2 and len(R({'layer_weights': 'exp'}, 8)) == 9
    lit = R({'layer_weights': '[0.4,0.3,0.2,0.1]'}, 3)
    assert np.array_equal(lit, np.array([0.4, 0.3, 0.2, 0.1], np.float32))                # verbatim: not normalised
    assert np.array_equal(R({'layer_weights': '[2, 0, 0, 3]'}, 3), np.array([2, 0, 0, 3], np.float32))
    assert np.array_equal(R({'layer_weights': [0.5, 0.5]}, 1), np.array([0.5, 0.5], np.float32))      # a config set from code
    for bad in ('[0.4,0.3,0.2]', '[0.4,0.3,0.2,0.1,0.0]', '[0.4,nan,0.2,0.1]', '[0.4,inf,0.2,0.1]', '[0,0,0,0]', '[1e39,0,0,0]',
                'median', '[0.4;0.3]', ''):
        with pytest.raises(ValueError, match="layer.weights"):
            R({'layer_weights': bad}, 3)
    with pytest.raises(ValueError, match="ppr_alpha"):
        R({'layer_weights': 'ppr', 'ppr_alpha': 0.0}, 3)
    with pytest.raises(ValueError, match="exp_smooth_beta"):
        R({'layer_weights': 'exp', 'exp_smooth_beta': float('nan')}, 3)


def test_ppr_flags_and_file_loader(pkg, tmp_path):
    R = pkg.model.resolve_layer_weights
    ppr = R({'layer_weights': 'ppr'}, 3)
    assert np.array_equal(R({'use_ppr_weights': True}, 3), ppr)                           # the flag alone means `ppr`
    assert np.array_equal(R({'use_ppr_weights': True, 'layer_weights': 'mean', 'ppr_alpha': 0.15}, 3), ppr)
    for other in ('exp', 'ppr', '[0.4,0.3,0.2,0.1]'):
        with pytest.raises(ValueError, match="use_ppr_weights.*layer_weights"):
            R({'use_ppr_weights': True, 'layer_weights': other}, 3)
    assert R({'ppr_weights_path': '/nonexistent.npy'}, 3) is None                         # as the reference: the path alone is not read
    # the file compute_ppr.py writes for `tiny` (tests/golden/make_ppr_golden.py: the reference's compute_ppr_weights, K = 3,
    # alpha = 0.15): [N, K+1] fp32, one row per node
    fixture = os.path.join(GOLDEN, "tiny", "ppr_weights.npy")
    W = np.load(fixture)
    z = np.load(os.path.join(GOLDEN, "tiny", "golden.npz"))
    deg = np.diff(z["adj_indptr"])
    assert W.shape == (len(deg), 4) and W.dtype == np.float32 and (deg == 0).sum() >= 1
    assert np.array_equal(W[deg == 0], np.tile(np.array([1, 0, 0, 0], np.float32), ((deg == 0).sum(), 1)))     # isolated: [1, 0, ...]
    got = R({'use_ppr_weights': True, 'ppr_weights_path': fixture}, 3, deg)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - ppr.astype(np.float64)).max() <= 1e-6
    with pytest.raises(ValueError, match="per-node weights are not implemented"):
        R({'use_ppr_weights': True, 'ppr_weights_path': fixture}, 3)                      # without the degrees the isolated row counts
    # a [K+1] file is taken as it is
    one = os.path.join(str(tmp_path), "one.npy")
    np.save(one, np.array([0.4, 0.3, 0.2, 0.1], np.float32))
    assert np.array_equal(R({'use_ppr_weights': True, 'ppr_weights_path': one}, 3, deg), np.array([0.4, 0.3, 0.2, 0.1], np.float32))
    # one connected node's row perturbed: per-node weights
    bad = os.path.join(str(tmp_path), "bad.npy")
    Wb = W.copy()
    node = int(np.flatnonzero(deg > 0)[5])
    Wb[node] = np.array([0.25, 0.25, 0.25, 0.25], np.float32)
    np.save(bad, Wb)
    with pytest.raises(ValueError, match="per-node weights are not implemented"):
        R({'use_ppr_weights': True, 'ppr_weights_path': bad}, 3, deg)
    # ... while an isolated node's row may be anything
    iso = os.path.join(str(tmp_path), "iso.npy")
    Wi = W.copy()
    Wi[deg == 0] = 0.25
    np.save(iso, Wi)
    assert np.array_equal(R({'use_ppr_weights': True, 'ppr_weights_path': iso}, 3, deg), got)
    # wrong shapes
    for arr in (W[:, :3], W[:-1], np.zeros((2, 2, 4), np.float32)):
        f = os.path.join(str(tmp_path), "shape.npy")
        np.save(f, arr)
        with pytest.raises(ValueError, match="ppr_weights_path"):
            R({'use_ppr_weights': True, 'ppr_weights_path': f}, 3, deg)


def _model(pkg, tmp_path, args, extra=None):
    d = os.path.join(str(tmp_path), "tiny")
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(GOLDEN, "tiny", f), os.path.join(d, f))
    w = pkg.world
    w.configure(["--dataset", "tiny", "--tensorboard", "0", "--layer", "3", "--recdim", "64", "--bpr_batch", "64"] + args)
    if extra:
        w.config.update(extra)
    ds = pkg.dataloader.Loader(w.config, path=d)
    return pkg.model.LightGCN(w.config, ds)


def test_refusals_need_no_device(pkg, tmp_path):
    L = pkg._lib
    fixture = os.path.join(GOLDEN, "tiny", "ppr_weights.npy")
    try:
        assert _model(pkg, tmp_path, []).layer_weights is None
        m = _model(pkg, tmp_path, ["--layer_weights", "exp"])
        assert np.array_equal(m.layer_weights, (np.array([8, 4, 2, 1], np.float64) / 15).astype(np.float32))
        ppr = _model(pkg, tmp_path, ["--use_ppr_weights"]).layer_weights
        assert np.array_equal(ppr, pkg.model.resolve_layer_weights({'layer_weights': 'ppr'}, 3))
        # the model hands the graph's degrees to the loader: the fixture's isolated node is ignored
        mf = _model(pkg, tmp_path, ["--use_ppr_weights", "--ppr_weights_path", fixture])
        assert np.abs(mf.layer_weights.astype(np.float64) - ppr.astype(np.float64)).max() <= 1e-6
        with pytest.raises(ValueError, match="layer weights"):
            _model(pkg, tmp_path, ["--layer_weights", "[0.5,0.5]"])                       # K = 3 needs four
        with pytest.raises(ValueError, match="use_ppr_weights.*layer_weights"):
            _model(pkg, tmp_path, ["--use_ppr_weights", "--layer_weights", "exp"])
        for flags, name in ((["--layer_weights", "exp"], "layer_weights"), (["--use_ppr_weights"], "use_ppr_weights")):
            with pytest.raises(L.LgcnError, match=name + ".*act_dtype fp8"):
                _model(pkg, tmp_path, flags + ["--act_dtype", "fp8"])
            with pytest.raises(L.LgcnError, match=name + ".*use_pop_gate"):
                _model(pkg, tmp_path, flags, extra={'use_pop_gate': True})
            with pytest.raises(L.LgcnError, match=name + ".*use_item_item"):
                _model(pkg, tmp_path, flags, extra={'use_item_item': True, 'i2i_alpha': 0.1,
                                                    'i2i_path': os.path.join(GOLDEN, "tiny", "i2i_tiny.npz")})
            with pytest.raises(L.LgcnError, match=name + ".*dropout 1"):
                _model(pkg, tmp_path, flags + ["--dropout", "1", "--keepprob", "0.6"])
        # data parallel: refused whatever the mode, before torch.distributed is even looked at
        for reduce, shard in (("rows", "batch"), ("dense", "batch"), ("rows", "rows"), ("rows", "cols")):
            with pytest.raises(RuntimeError, match="layer_weights"):
                pkg.parallel.DataParallelBPR(m, pkg.world.config, reduce=reduce, shard=shard)
    finally:
        pkg.world.configure([])
