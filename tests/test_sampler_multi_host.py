"""The device sampler for several negatives per positive (lgcn_sample_negative_device_multi; DESIGN 4 *Sampler*) without a
device: the two symbols, what the entry point refuses before it touches anything, the workspace query, and the host path of
Procedure.sample_epoch_to_device, which a CPU device keeps."""
import ctypes
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import storage_cases as SC                       # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402

NEW_SYMBOLS = ("lgcn_sample_negative_device_multi_workspace", "lgcn_sample_negative_device_multi")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13


def test_entry_point_refuses_before_touching_anything(pkg):
    """rc 3 for a negative ratio outside 1..16 (the message names it) and for null pointers; the output, the workspace and the
    host generator are as they were."""
    lib, npp = pkg._lib.load(), pkg._lib.npp
    indptr = np.array([0, 2, 4], np.int64)
    indices = np.array([0, 1, 1, 2], np.int32)
    out = np.full(64, -7, np.int32)
    work = np.full(1 << 12, 0x5a, np.uint8)

    def call(R, h=indptr, d_ip=indptr, d_ix=indices, S=out, ws=work):
        p = lambda a: npp(a) if a is not None else None
        return lib.lgcn_sample_negative_device_multi(2, 5, 8, p(h), p(d_ip), p(d_ix), R, p(S), p(ws), work.nbytes, None)

    pkg.sampling.seed(9)
    want = [pkg.sampling.randint(1 << 20) for _ in range(4)]
    pkg.sampling.seed(9)
    for R in (0, 17, -1):
        assert call(R) == 3 and b"negative ratio" in lib.lgcn_last_error(), R
        assert lib.lgcn_sample_negative_device_multi_workspace(2, 8, R) == 0
    for null in ("h", "d_ip", "d_ix", "S", "ws"):
        assert call(3, **{null: None}) == 3, null
    assert lib.lgcn_sample_negative_device_multi(0, 5, 8, npp(indptr), npp(indptr), npp(indices), 3, npp(out), npp(work), work.nbytes, None) == 3
    assert lib.lgcn_sample_negative_device_multi(2, 0, 8, npp(indptr), npp(indptr), npp(indices), 3, npp(out), npp(work), work.nbytes, None) == 3
    assert (out == -7).all() and (work == 0x5a).all()
    assert [pkg.sampling.randint(1 << 20) for _ in range(4)] == want


def test_workspace_query_grows_with_the_negative_ratio(pkg):
    lib = pkg._lib.load()
    for users, train in ((700, 13 * 700 + 5), (29858, 810128), (1, 1), (50, 49)):
        sizes = [int(lib.lgcn_sample_negative_device_multi_workspace(users, train, R)) for R in range(1, 17)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (users, train, sizes)
        assert sizes[0] >= int(lib.lgcn_sample_negative_device_workspace(users, train))
        if train >= users:                                       # the stream itself holds 1 + R draws per sample
            T = users * (train // users)
            assert all(s >= 4 * (1 + R) * T for R, s in zip(range(1, 17), sizes))
            assert T < 4092 or sizes[-1] > sizes[0]               # (the stream is whole blocks of 4 092 draws)
    # the margin hook serves both entry points
    try:
        before = int(lib.lgcn_sample_negative_device_multi_workspace(29858, 810128, 4))
        lib.lgcn_sampler_test_margin(1 << 40, 1)
        assert int(lib.lgcn_sample_negative_device_multi_workspace(29858, 810128, 4)) < before
    finally:
        lib.lgcn_sampler_test_margin(0, 0)
    assert int(lib.lgcn_sample_negative_device_multi_workspace(29858, 810128, 4)) == before


def _host_apply_perm_multi(S, s_cols, perm, T, users, pos, negs, R, stream):
    """lgcn_apply_perm_multi restated on host memory (the library's is a kernel: it cannot read the CPU tensors of this test)"""
    arr = lambda p, n, t: np.ctypeslib.as_array((t * n).from_address(p.value if hasattr(p, "value") else int(p)))
    S_ = arr(S, T * s_cols, ctypes.c_int32).reshape(T, s_cols)[arr(perm, T, ctypes.c_int64)]
    arr(users, T, ctypes.c_int32)[:] = S_[:, 0]
    arr(pos, T, ctypes.c_int32)[:] = S_[:, 1]
    arr(negs, R * T, ctypes.c_int32).reshape(R, T)[:] = S_[:, 2:2 + R].T
    return 0


def test_a_cpu_device_keeps_the_host_rows(pkg, storage_graph, monkeypatch):
    """Procedure.sample_epoch_to_device(ds, "cpu") with neg_ratio = 3 (gpu_sampler at its default 1): the device sampler is not
    called, and the host sampler's rows come back under the epoch permutation, negatives as [R, T]."""
    try:
        w = SC.configure(pkg, ("fp32", 32, 2, 1, -1, "propagated"), storage_graph)
        w.config['neg_ratio'] = 3
        w.config['sampler'] = 'cpp'
        assert int(w.config['gpu_sampler']) == 1
        ds = pkg.dataloader.Loader(w.config, path=storage_graph)

        def no_device(*a, **k):
            raise AssertionError("the device sampler was called for a CPU device")
        monkeypatch.setattr(pkg.sampling, "sample_negative_device", no_device)
        monkeypatch.setattr(pkg.sampling, "sample_negative_device_multi", no_device)
        monkeypatch.setattr(pkg._lib.load(), "lgcn_apply_perm_multi", _host_apply_perm_multi)
        monkeypatch.setattr(pkg._lib, "current_stream", lambda: None)
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        u, p, n = pkg.Procedure.sample_epoch_to_device(ds, "cpu")
        monkeypatch.undo()
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        S_ = np.asarray(pkg.sampling.sample_negative(ds.n_users, ds.m_items, ds.trainDataSize, pkg.utils._pos_csr(ds), 3))
        perm = pkg.utils.shuffle_indices(len(S_))
        assert n.shape == (3, len(S_)) and len(S_) > 0
        assert np.array_equal(u.numpy(), S_[perm, 0]) and np.array_equal(p.numpy(), S_[perm, 1])
        assert np.array_equal(n.numpy(), S_[perm, 2:].T)
    finally:
        pkg.world.configure([])
