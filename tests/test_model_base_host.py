"""model._TableModel, the base LightGCN and PureMF share: what needs no device.

The shared members are defined once and inherited; the two embedding weights stay views of ONE [N, d] table through a
state_dict load and .float() in both models (tests/test_mf_host.py::test_initial_weights_and_state_dict has the PureMF half
at construction); and LightGCN's refusals of option pairs come out first match first when several apply at once."""
import os
import re
import shutil

import pytest
import torch

from conftest import GOLDEN

SHARED = ("_rebind", "__del__", "_ids", "_fused_call", "check_device_errors", "adam_step", "set_adam_step", "_drop_device_state",
          "_state", "_dp_begin", "fused_step", "fused_epoch", "_retire_ctx", "_create_ctx", "_step_workspace", "_fill_step_config", "_bind_table",
          "_act", "_reg_ego", "_batch")
CTX_KEYS = {"destroy", "get_step", "set_step", "set_lr", "check", "step", "epoch"}


def _tiny(tmp_path):
    d = os.path.join(str(tmp_path), "tiny")
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(GOLDEN, "tiny", f), os.path.join(d, f))
    return d


def _model(pkg, tmp_path, cls, args=(), extra=None, seed=2020):
    w = pkg.world
    w.configure(["--dataset", "tiny", "--tensorboard", "0", "--layer", "2", "--recdim", "32", "--bpr_batch", "64"]
                + (["--model", "mf"] if cls == "PureMF" else []) + list(args))
    if extra:
        w.config.update(extra)
    ds = pkg.dataloader.Loader(w.config, path=_tiny(tmp_path))
    torch.manual_seed(seed)
    return ds, getattr(pkg.model, cls)(w.config, ds)


def test_shared_members_are_inherited(pkg):
    M = pkg.model
    base = M._TableModel
    assert issubclass(M.LightGCN, base) and issubclass(M.PureMF, base) and issubclass(base, torch.nn.Module)
    for cls in (M.LightGCN, M.PureMF):
        for name in SHARED:
            assert name in vars(base), name
            assert name not in vars(cls), (cls.__name__, name)
            assert getattr(cls, name) is getattr(base, name), (cls.__name__, name)
        # one small table names what differs between the two context types; every entry is an exported symbol
        assert set(cls._CTX) == CTX_KEYS and all(v in pkg._lib.SIGNATURES for v in cls._CTX.values()), cls.__name__
    assert not set(M.LightGCN._CTX.values()) & set(M.PureMF._CTX.values())
    # PureMF adds nothing to the single-storage machinery or to the fused calls; LightGCN extends _apply / _check_table
    # (the gate's tensors) and the dispatch (the negatives' shape), through the base's
    for name in ("_apply", "_check_table", "_dispatch", "invalidate_cache", "_open_state", "_ctx_rows", "_close_state"):
        assert name in vars(base) and name not in vars(M.PureMF) and name in vars(M.LightGCN), name
    for cls in (M.LightGCN, M.PureMF):              # each model's own: when a context is stale, how one is built
        assert "_ctx_stale" in vars(cls) and "_make_ctx" in vars(cls), cls.__name__


@pytest.mark.parametrize("cls", ["LightGCN", "PureMF"])
def test_single_storage_invariant_on_the_cpu(pkg, tmp_path, cls):
    """after a state_dict load and .float() the two weights are views of _table at offsets 0 and n_users d 4"""
    try:
        ds, m = _model(pkg, tmp_path, cls)
        d = m.latent_dim

        def bound(x):
            return (x._table.shape == (ds.n_users + ds.m_items, d) and x._table.dtype == torch.float32 and x._table.is_contiguous()
                    and x.embedding_user.weight.data_ptr() == x._table.data_ptr()
                    and x.embedding_item.weight.data_ptr() == x._table.data_ptr() + ds.n_users * d * 4)
        assert bound(m) and m._dev is None and m.adam_step == 0
        assert list(m.state_dict().keys())[:2] == ["embedding_user.weight", "embedding_item.weight"]
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        _, m2 = _model(pkg, tmp_path, cls, seed=7)
        assert not torch.equal(m2._table, m._table)
        m2.load_state_dict(sd)
        m2._check_table()
        assert bound(m2) and torch.equal(m2._table, m._table)
        assert m2.float() is m2 and bound(m2) and torch.equal(m2._table, m._table)
        # a weight somebody replaced by an independent tensor is copied back into the table and rebound
        with torch.no_grad():
            m2.embedding_item.weight.data = torch.full((ds.m_items, d), 0.25)
        assert not bound(m2)
        m2._check_table()
        assert bound(m2) and bool((m2._table[ds.n_users:] == 0.25).all()) and torch.equal(m2._table[:ds.n_users], m._table[:ds.n_users])
        # a dtype round trip makes a new table: both views follow it, and the device state would be dropped with the old one
        m2.double()
        assert m2._table.dtype == torch.float64 and m2.embedding_user.weight.data_ptr() == m2._table.data_ptr()
        m2.float()
        assert bound(m2) and m2._dev is None
        # the config accessors read when they are called
        assert (m._act(), m._reg_ego(), m._batch(7)) == ("fp32", False, 64)
        m.config.update({'act_dtype': 'bf16', 'reg_rows': 'ego', 'bpr_batch_size': 48})
        assert (m._act(), m._reg_ego(), m._batch(7)) == ("bf16", True, 48)
        del m.config['bpr_batch_size']
        assert m._batch(7) == 7
    finally:
        pkg.world.configure([])


GATE = {'use_pop_gate': True}
REFUSALS = [
    # (flags, config entries, the text of the first refusal that applies)
    (["--dropout", "1", "--act_dtype", "fp8"], None,
     "--dropout 1 is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)"),
    (["--dropout", "1", "--act_dtype", "fp8", "--layer_weights", "exp", "--neg_ratio", "2"], None,          # ... before layer weights / fp8
     "--dropout 1 is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)"),
    (["--act_dtype", "fp8", "--layer_weights", "exp"], None,
     "--layer_weights is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)"),
    (["--act_dtype", "fp8", "--layer_weights", "exp", "--neg_ratio", "2", "--loss", "softmax"], None,       # ... before neg_ratio / fp8, loss / fp8
     "--layer_weights is not implemented together with --act_dtype fp8 (fp32 and bf16 storage only)"),
    (["--neg_ratio", "2"], GATE,
     "--neg_ratio 2 is not implemented together with --use_pop_gate / --use_item_item (the optional branches train on one negative per positive)"),
    (["--neg_ratio", "2", "--loss", "softmax"], GATE,                                                       # ... before loss / gate
     "--neg_ratio 2 is not implemented together with --use_pop_gate / --use_item_item (the optional branches train on one negative per positive)"),
]


@pytest.mark.parametrize("args,extra,text", REFUSALS, ids=[" ".join(a).replace("--", "") + ("+gate" if e else "") for a, e, _ in REFUSALS])
def test_refusals_come_first_match_first(pkg, tmp_path, args, extra, text):
    try:
        with pytest.raises(pkg._lib.LgcnError, match="^" + re.escape(text) + "$"):
            _model(pkg, tmp_path, "LightGCN", args, extra)
    finally:
        pkg.world.configure([])
