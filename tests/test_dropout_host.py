"""Edge dropout (--dropout, --keepprob): everything that needs no device -- the ABI surface, the flags' way into the
config, and the refusals that must be raised before any device call."""
import os
import re
import shutil

import pytest

from conftest import GOLDEN, REPO

NEW_SYMBOLS = ("lgcn_ctx_set_dropout", "lgcn_dropout_mask", "lgcn_spmm_csr_drop")


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
    assert lib.lgcn_ctx_set_dropout(None, 0.6, 1) == 3
    assert lib.lgcn_dropout_mask(None, None, 0, 0, 0.6, 1, 0, None, None) == 3
    assert lib.lgcn_spmm_csr_drop(None, None, 0, None, 0, 64, 0.6, 1, 0, 0, None) == 3


def test_flags_reach_the_config(pkg):
    w = pkg.world
    try:
        w.configure(['--dropout', '1', '--keepprob', '0.6'])
        assert w.config['dropout'] == 1 and w.config['keep_prob'] == 0.6 and w.config['seed'] == 2020
        w.configure([])
        assert w.config['dropout'] == 0
    finally:
        w.configure([])


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
    import torch
    L = pkg._lib
    try:
        m = _model(pkg, tmp_path, ["--dropout", "1", "--keepprob", "0.6"])
        assert m.dropout and abs(m.keep_prob - 0.6) < 1e-12
        assert not _model(pkg, tmp_path, ["--keepprob", "0.6"]).dropout                   # --dropout 0: the knob alone does nothing
        for bad in ("0", "-0.1", "1.5", "nan"):
            with pytest.raises(ValueError, match="keepprob"):
                _model(pkg, tmp_path, ["--dropout", "1", "--keepprob", bad])
        _model(pkg, tmp_path, ["--dropout", "0", "--keepprob", "1.5"])                    # ... and is not looked at when dropout is off
        _model(pkg, tmp_path, ["--dropout", "1", "--keepprob", "1.0"])                    # 1.0 is in range (off)
        with pytest.raises(L.LgcnError, match="dropout.*act_dtype fp8"):
            _model(pkg, tmp_path, ["--dropout", "1", "--act_dtype", "fp8"])
        with pytest.raises(L.LgcnError, match="dropout.*use_pop_gate"):
            _model(pkg, tmp_path, ["--dropout", "1"], extra={'use_pop_gate': True})
        with pytest.raises(L.LgcnError, match="dropout.*use_item_item"):
            _model(pkg, tmp_path, ["--dropout", "1"], extra={'use_item_item': True, 'i2i_alpha': 0.1,
                                                              'i2i_path': os.path.join(GOLDEN, "tiny", "i2i_tiny.npz")})
        # data parallel: refused whatever the mode, before torch.distributed is even looked at
        for reduce, shard in (("rows", "batch"), ("dense", "batch"), ("rows", "rows"), ("rows", "cols")):
            with pytest.raises(RuntimeError, match="dropout"):
                pkg.parallel.DataParallelBPR(m, pkg.world.config, reduce=reduce, shard=shard)
        # the unfused autograd path: computer() in training mode with gradients enabled, i.e. model.bpr_loss
        m.train()
        ids = torch.zeros(4, dtype=torch.long)
        with pytest.raises(RuntimeError, match="dropout"):
            m.bpr_loss(ids, ids, ids)
        with pytest.raises(RuntimeError, match="dropout"):
            m.computer()
    finally:
        pkg.world.configure([])
