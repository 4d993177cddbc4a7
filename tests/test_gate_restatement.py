"""CPU side of the gated / smoothed fused step's tests: the float64 restatement of the step (tests/gate_restatement.py) against
the fixtures recorded from the reference with the branches on (tests/golden/tiny/golden_{gate,i2i,gate_i2i,gate_i2i_k1,_k2,_k4}),
at the tolerances test_optional_branches_vs_reference_golden uses for the same quantities -- so the restatement IS the
reference's model before tests/test_gpu_gate_shapes.py judges a kernel by it.  Then the shapes of that GPU test (CASES, the
two graph geometries, the batches) with the conditions its inputs must meet, checked here from the CPU references alone, and
the boundary of LightGCN.fused_variants.

Here every step of a case starts from the float64 trajectory (restated loss, gradients, Adam), rounded to fp32; the GPU test
asserts the same conditions again at the states its own steps start from."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import gate_restatement as R                     # noqa: E402
from conftest import GOLDEN, read_interactions   # noqa: E402
from gate_cases import (BAD_ID_CASES, BAD_IDS, CASES, GEOMETRY, bad_id_batch, case_id, cpu_trajectory, make_batches, make_model,  # noqa: E402
                        model_inputs, references, step_bounds, storage_allowance)
from gate_cases import graph_dirs                # noqa: E402,F401  (fixture: both graphs, written once per session)

TINY = os.path.join(GOLDEN, "tiny")
TAGS = ("gate", "i2i", "gate_i2i", "gate_i2i_k1", "gate_i2i_k2", "gate_i2i_k4")


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement against the reference's fixtures
def _tiny_inputs(meta, gz):
    users, items = read_interactions(os.path.join(TINY, "train.txt"))
    n_users, m_items = gz["P0.embedding_user.weight"].shape[0], gz["P0.embedding_item.weight"].shape[0]
    adj = R.norm_adj(n_users, m_items, users, items)
    counts = np.bincount(items, minlength=m_items).astype(np.float64)
    counts[counts == 0] = 1.0                                        # (the dataset object's items_D)
    i2i = None
    if meta["use_item_item"]:
        m = sp.load_npz(os.path.join(TINY, "i2i_tiny.npz")).tocsr().astype(np.float32)
        m.data = (np.float32(meta["i2i_alpha"]) * m.data).astype(np.float32)
        i2i = m
    return dict(adj=adj, pop=R.pop_scalar(counts) if meta["use_pop_gate"] else None, i2i=i2i, n_users=n_users, K=meta["K"],
                decay=meta["decay"], temp=meta["pop_gate_temp"], coeff=meta["gate_entropy_coeff"])


def _params(gz, prefix, gate):
    table = np.concatenate([gz[prefix + "embedding_user.weight"], gz[prefix + "embedding_item.weight"]], 0)
    return table, ([gz[prefix + k] for k in R.MLP_NAMES] if gate else None)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    """loss / reg of the reference's first batch (2e-6), the gradient of EVERY parameter (rtol 5e-4, atol 2e-8), then three
    restated Adam steps: their losses (5e-6) and every parameter afterwards (2e-5)."""
    gz = np.load(os.path.join(TINY, f"golden_{tag}.npz"))
    meta = json.load(open(os.path.join(TINY, f"golden_{tag}.json")))
    gate = bool(meta["use_pop_gate"])
    inp = _tiny_inputs(meta, gz)
    table, mlp = _params(gz, "P0.", gate)
    b = gz["batches"]
    r = R.step(table=table, mlp=mlp, batch=tuple(b[0]), **inp)
    assert abs(r["loss"] - meta["b_loss"]) < 2e-6 and abs(r["reg"] - meta["b_reg"]) < 2e-6 and abs(r["total"] - meta["b_total"]) < 2e-6
    nu = inp["n_users"]
    np.testing.assert_allclose(r["grad_table"][:nu], gz["G0.embedding_user.weight"], rtol=5e-4, atol=2e-8)
    np.testing.assert_allclose(r["grad_table"][nu:], gz["G0.embedding_item.weight"], rtol=5e-4, atol=2e-8)
    for k, g in zip(R.MLP_NAMES, r["grad_mlp"]):
        np.testing.assert_allclose(g, gz["G0." + k], rtol=5e-4, atol=2e-8, err_msg=k)
    if gate:
        assert r["pre_pop"].shape == (2 * b.shape[2], meta["pop_hidden"]) and r["pre_gate"].shape == (2 * b.shape[2], meta["gate_hidden"])
        assert r["gates"].shape == (2 * b.shape[2],) and (r["gates"] > 0).all() and (r["gates"] < 1).all()
    # three steps of torch.optim.Adam over all parameters, from the initial ones
    ps = [table.astype(np.float64)] + ([np.asarray(t, np.float64) for t in mlp] if gate else [])
    ms, vs = [np.zeros_like(t) for t in ps], [np.zeros_like(t) for t in ps]
    for i in range(3):
        r = R.step(table=ps[0], mlp=ps[1:] if gate else None, batch=tuple(b[i + 1]), **inp)
        assert abs(r["total"] - meta["step_losses"][i]) < 5e-6, (i, r["total"], meta["step_losses"][i])
        gs = [r["grad_table"]] + r["grad_mlp"]
        for j in range(len(ps)):
            ps[j], ms[j], vs[j] = R.adam(ps[j], ms[j], vs[j], gs[j], i + 1, meta["lr"])
    want_table, want_mlp = _params(gz, "P3.", gate)
    np.testing.assert_allclose(ps[0], want_table, rtol=0, atol=2e-5)
    for k, got, want in zip(R.MLP_NAMES, ps[1:], want_mlp or []):
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5, err_msg=k)


def test_fp32_twin_is_the_same_code():
    """dtype=float32 runs the same statements: on the gate_i2i fixture it lands within fp32 rounding of float64 (far inside the
    fixture tolerances), and it is not the float64 result."""
    gz = np.load(os.path.join(TINY, "golden_gate_i2i.npz"))
    meta = json.load(open(os.path.join(TINY, "golden_gate_i2i.json")))
    inp = _tiny_inputs(meta, gz)
    table, mlp = _params(gz, "P0.", True)
    r64 = R.step(table=table, mlp=mlp, batch=tuple(gz["batches"][0]), **inp)
    r32 = R.step(table=table, mlp=mlp, batch=tuple(gz["batches"][0]), dtype=torch.float32, **inp)
    assert 0.0 < abs(r32["loss"] - r64["loss"]) < 2e-6 and abs(r32["reg"] - r64["reg"]) < 2e-6
    assert 0.0 < R.rel_max(r32["grad_table"], r64["grad_table"]) < 5e-4
    for a, b_ in zip(r32["grad_mlp"], r64["grad_mlp"]):
        assert R.rel_max(a, b_) < 5e-4


# ---------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_gate_shapes.py (tests/gate_cases.py)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_inputs_meet_their_conditions_on_the_cpu(pkg, graph_dirs, case):
    """Every step of every GPU case, from the CPU references alone: kink and clamp margins, saturation shares, visibility of the
    entropy term and of the temperature (all asserted inside references()); the figures are printed."""
    try:
        ds, m = make_model(pkg, case, graph_dirs[case[8]])
        n_users, m_items = GEOMETRY[case[8]]
        assert (ds.n_users, ds.m_items) == (n_users, m_items)
        deg = np.diff(ds.getSparseGraphCSR().indptr)
        assert deg[:n_users].max() == 150 and deg[:n_users].min() >= 1 and sorted(set(deg[:n_users].tolist()) - {150}) == list(range(1, 20))
        inp = model_inputs(case, ds, m)
        # what the package built on this graph against the restatement's own: the adjacency (structure exactly; values to 2 fp32
        # ulps: D^-1/2 A D^-1/2 multiplied in another order), the popularity scalar and alpha * I2I exactly
        tu, ti = read_interactions(os.path.join(graph_dirs[case[8]], "train.txt"))
        own, got = R.norm_adj(n_users, m_items, tu, ti), inp["adj"]
        assert np.array_equal(own.indptr, got.indptr) and np.array_equal(own.indices, got.indices)
        assert (np.abs(own.data.astype(np.float64) - got.data) <= 2.0 ** -22 * np.abs(own.data)).all()
        if case[6]:
            counts = np.bincount(ti, minlength=m_items).astype(np.float64)
            counts[counts == 0] = 1.0
            assert np.array_equal(R.pop_scalar(counts), inp["pop"])
        if case[7]:
            file = sp.load_npz(os.path.join(graph_dirs[case[8]], "i2i.npz")).tocsr().astype(np.float32)
            file.sort_indices()
            assert np.array_equal(file.indptr, inp["i2i"].indptr) and np.array_equal(file.indices, inp["i2i"].indices)
            assert np.array_equal((np.float32(0.3) * file.data).astype(np.float32), inp["i2i"].data)
        mlp = [p.detach().numpy().copy() for p in m.gate_parameters()] if case[6] else None
        batches = make_batches(case, n_users, m_items)
        states = cpu_trajectory(case, inp, m._table.numpy().copy(), mlp, batches)
        for i, (batch, (ps, _, _)) in enumerate(zip(batches, states)):
            r64, e32, info = references(case, inp, ps[0], ps[1:] if case[6] else None, batch, i + 1)
            b = step_bounds(e32, r64, len(batch[0]))
            assert all(0.0 < b[k] <= 2e-6 for k in ("loss", "reg", "total")) and 0.0 < b["table"] <= 5e-4 and all(0.0 <= v <= 5e-4 for v in b["mlp"])
            print(f"{case_id(case)} step {i + 1} B={len(batch[0])}: e32 loss {e32['loss']:.1e} reg {e32['reg']:.1e} table {e32['table']:.1e} "
                  f"mlp {max(e32['mlp'], default=0.0):.1e} " + " ".join(f"{k}={v}" for k, v in info.items()))
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("which", range(len(BAD_IDS)), ids=[b[0] for b in BAD_IDS])
@pytest.mark.parametrize("case", BAD_ID_CASES, ids=case_id)
def test_bad_id_batches_meet_their_conditions_on_the_cpu(pkg, graph_dirs, case, which):
    """The 15 sound triplets of the bad-id batches, at the initial parameters (the GPU test takes one step from them)."""
    try:
        ds, m = make_model(pkg, case, graph_dirs[case[8]])
        batch, sound = bad_id_batch(case, which)
        bad = [np.flatnonzero((batch[0] < 0) | (batch[0] >= ds.n_users)), np.flatnonzero((batch[1] < 0) | (batch[1] >= ds.m_items)),
               np.flatnonzero((batch[2] < 0) | (batch[2] >= ds.m_items))]
        assert sorted(np.concatenate(bad).tolist()) == [5] and bad[BAD_IDS[which][1]].tolist() == [5] and len(sound[0]) == 15
        mlp = [p.detach().numpy().copy() for p in m.gate_parameters()]
        _, e32, info = references(case, model_inputs(case, ds, m), m._table.numpy().copy(), mlp, sound, 1)
        print(f"{case_id(case)} {BAD_IDS[which][0]}: e32 loss {e32['loss']:.1e} reg {e32['reg']:.1e} table {e32['table']:.1e} "
              f"mlp {max(e32['mlp']):.1e} " + " ".join(f"{k}={v}" for k, v in info.items()))
    finally:
        pkg.world.configure([])


def test_bf16_storage_allowance_against_an_exact_backward_chain(pkg, graph_dirs):
    """No kernel: the float64 gradient rows of the bf16 case pushed through the backward chain h_K = Gs, h_{k-1} = Gs + A h_k with
    its K - 1 intermediate tables rounded to bf16 (round to nearest even) and nothing else inexact.  What storage alone costs is
    not small (> 1e-4 of the tensor's max, against 8 e32 ~ 1e-5), every element of it stays inside storage_allowance() -- the
    bound the GPU test adds for this case is one a correct implementation meets -- and the same expression with 2^-9 in the
    place of 2^-8 is exceeded by this exact chain."""
    case = [c for c in CASES if c[9] == "bf16"][0]
    K = case[1]
    bf = lambda x: torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).double().numpy()      # noqa: E731
    try:
        ds, m = make_model(pkg, case, graph_dirs[case[8]])
        inp = model_inputs(case, ds, m)
        mlp = [p.detach().numpy().copy() for p in m.gate_parameters()]
        batches = make_batches(case, ds.n_users, ds.m_items)
        A = inp["adj"].astype(np.float64)
        share = 0.0
        for i, (batch, (ps, _, _)) in enumerate(zip(batches, cpu_trajectory(case, inp, m._table.numpy().copy(), mlp, batches))):
            r = R.step(table=ps[0], mlp=ps[1:], batch=batch, **inp)
            gs = r["grad_final"] / (K + 1)
            h = gs
            for k in range(K, 0, -1):
                h = gs + A @ h
                if k > 1:
                    h = bf(h)
            err = np.abs(h - r["grad_table"])
            allow = storage_allowance(inp["adj"], r["grad_final"], K)
            raw = float(err.max() / np.abs(r["grad_table"]).max())
            used = float((err / np.maximum(allow, 1e-300)).max())
            share = max(share, used)
            print(f"{case_id(case)} step {i + 1}: an exact chain with bf16 tables is {raw:.1e} of the max away; largest share of the allowance {used:.2f}")
            assert raw > 1e-4 and (err <= allow).all(), (i, raw, used)
        assert 0.5 < share <= 1.0, share          # (more than half: 2^-9 in the place of 2^-8 would not hold)
    finally:
        pkg.world.configure([])


def test_fused_variants_boundary(pkg, graph_dirs):
    """pop_hidden 64 / gate_hidden 64 / d 128 is the largest gate the fused step holds; 65, 65, d 256 and a temperature <= 0 fall
    back to the autograd path, and fused_step then raises the documented RuntimeError."""
    base = (128, 1, 64, 64, 1.0, 0.05, True, False, "A", "fp32")
    try:
        ds, m = make_model(pkg, base, graph_dirs["A"])
        assert m.has_variants and m.fused_variants and pkg.utils.BPRLoss(m, pkg.world.config).fused
        for change in ({2: 65}, {3: 65}, {0: 256}, {4: 0.0}, {4: -1.0}):
            case = tuple(change.get(i, v) for i, v in enumerate(base))
            ds, m = make_model(pkg, case, graph_dirs["A"])
            assert m.has_variants and not m.fused_variants, change
            assert not pkg.utils.BPRLoss(m, pkg.world.config).fused, change
            ids = torch.zeros(4, dtype=torch.int64)
            with pytest.raises(RuntimeError, match="outside the fused step"):
                m.fused_step(ids, ids, ids)
            with pytest.raises(RuntimeError, match="outside the fused step"):
                m.fused_epoch(ids, ids, ids, 4)
        ds, m = make_model(pkg, base, graph_dirs["A"], fused=0)
        assert not m.fused_variants
        with pytest.raises(RuntimeError, match="outside the fused step"):
            m.fused_step(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    finally:
        pkg.world.configure([])
