"""The shapes of tests/test_gpu_gate_shapes.py and what it shares with tests/test_gate_restatement.py: the cases, the two graph
geometries, the batches and their seeds, model construction, the float64 / fp32-twin references of a step with the conditions
its inputs must meet, and the bounds.  Test infrastructure like tests/gate_restatement.py, which holds the arithmetic."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gate_restatement as R

GEOMETRY = {"A": (157, 223),        # the item block starts mid-word in the row bitmap and N = 380 ends mid-word
            "B": (160, 224)}        # both edges on word boundaries (k_flag_range's  hi & 31 == 0  arm)
ALPHA, LR, DECAY, MODEL_SEED = 0.3, 1e-3, 1e-4, 2020
BATCH_SIZES = (64, 37, 9, 1)        # partial workgroups of GATE_TPB = 8 triplets, and a one-triplet batch
SAT_TEMP = 2.0 ** -8                # saturation case: 40 - 80 % of a batch's gates leave the clamp's range (2^-7: < 10 %, 2^-9: > 90 %); 1 / T is exact
# (d, K, pop_hidden, gate_hidden, temperature, entropy coefficient, gate, i2i, geometry, activation storage)
CASES = [(32, 2, 32, 64, 1.0, 1e-4, True, True, "A", "fp32"),
         (32, 1, 17, 33, 0.25, 0.05, True, False, "B", "fp32"),
         (64, 3, 17, 33, 0.25, 0.05, True, True, "A", "fp32"),
         (64, 2, 32, 64, SAT_TEMP, 0.05, True, False, "A", "fp32"),
         (128, 1, 64, 64, 1.0, 0.05, True, False, "A", "fp32"),
         (128, 4, 1, 1, 2.0, 0.05, True, True, "B", "fp32"),
         (128, 3, 32, 64, 1.0, 0.05, True, True, "A", "bf16"),
         (32, 3, 32, 64, 1.0, 1e-4, False, True, "A", "fp32"),
         (128, 2, 32, 64, 1.0, 1e-4, False, True, "B", "fp32")]
# seed of a case's batches: 0 unless one of the conditions below fails there (found on the CPU, with this file alone)
BATCH_SEED = {"d32-K2-H32x64-T1-c0.0001-gate+i2i-A": 2,          # seeds 0, 1: a pop_mlp unit 1.8e-6 from its kink (13 twin errors)
              "d64-K2-H32x64-T0.00390625-c0.05-gate-A": 1,       # seed 0: a gate 7 twin errors from the clamp's edge in step 2
              "d128-K3-H32x64-T1-c0.05-gate+i2i-A-bf16": 1}      # seed 0: a gate_mlp unit 7.0e-6 from its kink (4 twin errors, bf16 layers)
KINK_FACTOR = 16.0                  # a pre-activation / a gate counts as decided when it is 16 twin errors away from the kink / the clamp edge
BOUND_FACTOR = 8.0                  # the GPU may be 8 twin errors away from float64 (summation order, lane reductions, one 2^-50 rounding)
CAP = {"loss": 2e-6, "reg": 2e-6, "total": 2e-6, "grad": 5e-4}       # the project's tolerances for the same quantities on this path


def case_id(c):
    d, K, Hp, Hg, temp, coeff, gate, i2i, geo, act = c
    return f"d{d}-K{K}-" + (f"H{Hp}x{Hg}-T{temp:g}-c{coeff:g}-" if gate else "") + ("gate" if gate else "") + ("+" if gate and i2i else "") + \
        ("i2i" if i2i else "") + f"-{geo}" + ("-bf16" if act == "bf16" else "")


def write_graph(path, geo, seed=5):
    """train.txt / test.txt / i2i.npz of a geometry: degrees 1..19, every 37th user 150 items (one row beyond a unit of 128
    non-zeros); a 5 % dense item-item matrix with every 11th row empty and two items that appear in no row."""
    n_users, m_items = GEOMETRY[geo]
    rng = np.random.Generator(np.random.PCG64(seed))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(n_users):
            k = int(rng.integers(1, 20)) if u % 37 else 150
            items = np.sort(rng.choice(m_items, size=k, replace=False))
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {int(rng.integers(0, m_items))}\n")
    m = sp.random(m_items, m_items, density=0.05, random_state=np.random.RandomState(seed), format="lil", dtype=np.float64)
    for r in range(0, m_items, 11):
        m.rows[r], m.data[r] = [], []
    m = m.tocsc()
    for c in (5, m_items - 1):
        m.data[m.indptr[c]:m.indptr[c + 1]] = 0.0
    m.eliminate_zeros()
    m = m.tocsr().astype(np.float32)
    m.sort_indices()
    nnz_row, nnz_col = np.diff(m.indptr), np.diff(m.tocsc().indptr)
    assert (nnz_row[::11] == 0).all() and nnz_col[5] == 0 and nnz_col[m_items - 1] == 0 and (nnz_row > 0).sum() > m_items // 2
    sp.save_npz(os.path.join(path, "i2i.npz"), m)
    return n_users, m_items


def make_batches(case, n_users, m_items):
    rng = np.random.Generator(np.random.PCG64(1000 * BATCH_SEED.get(case_id(case), 0) + case[0] + case[1]))
    out = []
    for nb in BATCH_SIZES:
        u = rng.integers(0, n_users, nb); p = rng.integers(0, m_items, nb); n = rng.integers(0, m_items, nb)
        if nb > 8:
            p[:4] = p[4]; n[5] = p[4]; u[7] = u[6]
        out.append((u, p, n))
    return out


# an out-of-range id in slot 5 of a 16-triplet batch (tests/test_gpu_gate_shapes.py): (name, which id array, the id)
BAD_IDS = (("user_is_n_users", 0, "n_users"), ("pos_is_m_items", 1, "m_items"), ("neg_is_minus_one", 2, -1))
BAD_ID_CASES = [CASES[4], CASES[1]]          # d = 128 and d = 32, gate only, geometry A and B
BAD_ID_SEED = {}                             # as BATCH_SEED


def bad_id_batch(case, which):
    """-> (the batch with the bad id, the 15 sound triplets)."""
    n_users, m_items = GEOMETRY[case[8]]
    rng = np.random.Generator(np.random.PCG64(77 + 1000 * BAD_ID_SEED.get((case_id(case), which), 0) + case[0] + which))
    u = rng.integers(0, n_users, 16); p = rng.integers(0, m_items, 16); n = rng.integers(0, m_items, 16)
    p[:4] = p[4]; n[6] = p[4]; u[8] = u[7]
    keep = np.arange(16) != 5
    sound = (u[keep].copy(), p[keep].copy(), n[keep].copy())
    ids = [u, p, n]
    _, col, bad = BAD_IDS[which]
    ids[col][5] = {"n_users": n_users, "m_items": m_items}.get(bad, bad)
    return tuple(ids), sound


def configure(pkg, case, path, fused=1, batch=64):
    d, K, Hp, Hg, temp, coeff, gate, i2i, geo, act = case
    w = pkg.world
    w.configure([])
    w.dataset = "gate_shapes"
    w.config.update({'lightGCN_n_layers': K, 'latent_dim_rec': d, 'bpr_batch_size': batch, 'decay': DECAY, 'lr': LR, 'act_dtype': act,
                     'use_pop_gate': gate, 'pop_hidden': Hp, 'gate_hidden': Hg, 'pop_gate_temp': temp, 'gate_entropy_coeff': coeff,
                     'use_item_item': i2i, 'i2i_path': os.path.join(path, "i2i.npz") if i2i else None, 'i2i_alpha': ALPHA if i2i else 0.0,
                     'fused_variants': fused, 'checkpoint_dir': os.path.join(path, "ckpt")})
    return w


def make_model(pkg, case, path, fused=1, batch=64):
    """The dataset and a fresh CPU model of a case (seed MODEL_SEED); the caller moves it to the device and resets world's config."""
    w = configure(pkg, case, path, fused, batch)
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(MODEL_SEED)
    m = pkg.model.LightGCN(w.config, ds)
    m.train()
    return ds, m


def model_inputs(case, ds, m):
    """What the restatement needs besides the parameters, taken from the dataset / model objects as the fused step gets them."""
    d, K, Hp, Hg, temp, coeff, gate, i2i, geo, act = case
    i2 = None
    if i2i:
        i2 = m._i2i.copy()
        i2.data = (np.float32(m.i2i_alpha) * i2.data).astype(np.float32)
    return dict(adj=ds.getSparseGraphCSR(), pop=m.item_pop_scalar.cpu().numpy() if gate else None, i2i=i2, n_users=ds.n_users, K=K,
                decay=DECAY, temp=temp, coeff=coeff, act_bf16=(act == "bf16"))


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def references(case, inp, table, mlp, batch, step_no):
    """float64 reference and fp32 twin of one step at the given (fp32) parameters -> (r64, e32, info), and the conditions on the
    inputs, asserted: ReLU kinks and clamp edges decided, the saturation shares of the saturation case, the entropy term and the
    temperature visible.  e32: the twin's distance from float64, {'loss', 'reg', 'total', 'table', 'mlp': [8]}, gradients as
    fractions of the float64 tensor's max."""
    cid, gate = case_id(case), case[6]
    r64 = R.step(table=table, mlp=mlp, batch=batch, **inp)
    r32 = R.step(table=table, mlp=mlp, batch=batch, dtype=torch.float32, **inp)
    e32 = {k: abs(r32[k] - r64[k]) for k in ("loss", "reg", "total")}
    e32["table"] = R.rel_max(r32["grad_table"], r64["grad_table"])
    e32["mlp"] = [R.rel_max(a, b) for a, b in zip(r32["grad_mlp"], r64["grad_mlp"])]
    info = {}
    if gate:
        pre64 = np.concatenate([r64["pre_pop"].ravel(), r64["pre_gate"].ravel()])
        pre32 = np.concatenate([r32["pre_pop"].ravel(), r32["pre_gate"].ravel()])
        e_pre, margin = float(np.abs(pre32 - pre64).max()), float(np.abs(pre64).min())
        info["kink"] = f"{margin:.1e}/{e_pre:.1e}"
        assert margin >= KINK_FACTOR * e_pre, ("a hidden unit sits on its ReLU kink: pick another batch seed for this case", cid, step_no, margin, e_pre)
        # the clamp's edges, gate by gate: a saturated gate is within 1e-6 of its edge by definition, so the distance is measured
        # in the gate's own twin error
        g64, e_g = r64["gates"], np.abs(r32["gates"] - r64["gates"])
        edge = np.minimum(np.abs(g64 - R.CLAMP), np.abs(g64 - (1.0 - R.CLAMP)))
        sat = float(((g64 < R.CLAMP) | (g64 > 1.0 - R.CLAMP)).mean())
        info["saturated"] = f"{sat:.2f}"
        info["edge"] = f"{float((edge / np.maximum(e_g, 1e-300)).min()):.1e}"
        assert (edge >= KINK_FACTOR * e_g).all(), ("a gate sits on the clamp's edge: pick another batch seed for this case", cid, step_no,
                                                   float((edge / np.maximum(e_g, 1e-300)).min()))
        if case[4] == SAT_TEMP and len(batch[0]) >= 9:          # (a batch of one triplet has two gates: no 10 % shares to speak of)
            assert 0.1 <= sat <= 0.9, ("saturation case: at least 10 % of the gates outside the clamp's range and 10 % inside: "
                                       "pick another batch seed for this case", cid, step_no, sat)
        if step_no == 1 and case[5] == 0.05:
            # would the comparison notice a kernel that drops the entropy gradient, or ignores 1 / T?  The float64 gradient without
            # the term differs from the true one by more than 100 x the LARGEST bound a gradient tensor can have here (CAP)
            alts = {"coeff=0": dict(inp, coeff=0.0)}
            if case[4] != 1.0:
                alts["T=1"] = dict(inp, temp=1.0)
            for what, alt in alts.items():
                ra = R.step(table=table, mlp=mlp, batch=batch, **alt)
                vis = max(R.rel_max(a, b) for a, b in zip(ra["grad_mlp"], r64["grad_mlp"]) if np.abs(b).max() > 0)
                info[what] = f"{vis:.2g}"
                assert vis > 100.0 * CAP["grad"], ("the term is invisible at this case's bound", cid, what, vis)
    return r64, e32, info


def step_bounds(e32, r64, n_triplets):
    """The bounds of ONE step from the twin's distances of that step: the GPU may be BOUND_FACTOR x e32 away from float64.
    A quantity that is ONE fp32 number gets a floor under that, because its e32 is a single rounding-error sample and can fall
    anywhere below the resolution of the format, while no fp32 evaluation can be expected to.  Such a quantity is a sum of n
    terms that are themselves fp32 results: each term carries at least one rounding of its own, 2^-24 |term| counting its last
    operation and the operand before it, and the most accurate fixed order a wave has for adding n fp32 numbers, a binary tree,
    rounds ceil(log2 n) partial sums, none larger than sum |term|:   floor = (1 + ceil(log2 n)) 2^-24 sum |term|.
      loss / reg / total: n = B triplets, every term of one sign, so sum |term| = |value| (1 to 7 fp32 ulps of the value for
        B = 1 ... 64);
      a one-element gradient (gate_mlp.2.bias always; any MLP tensor of a hidden layer of width 1): n = 2B slots,
        sum |term| from the restatement (grad_mlp_abs), as a fraction of |value| like every gradient distance here -- dlogit has
        both signs, so this can be many ulps of a cancelling sum.  (The kernel adds these terms exactly, in fixed point; the
        terms are products of four to six fp32 results each.)
    Every bound stays capped at the project's tolerance for the quantity (CAP)."""
    tree = lambda n: (1 + int(np.ceil(np.log2(n)))) * 2.0 ** -24      # noqa: E731
    b = {k: min(max(BOUND_FACTOR * e32[k], tree(n_triplets) * abs(r64[k])), CAP[k]) for k in ("loss", "reg", "total")}
    b["table"] = min(BOUND_FACTOR * e32["table"], CAP["grad"])
    b["mlp"] = []
    for e, g, terms in zip(e32["mlp"], r64["grad_mlp"], r64.get("grad_mlp_abs", [])):
        one = g.size == 1 and float(g.ravel()[0]) != 0.0
        floor = tree(2 * n_triplets) * float(terms.ravel()[0]) / abs(float(g.ravel()[0])) if one else 0.0
        b["mlp"].append(min(max(BOUND_FACTOR * e, floor), CAP["grad"]))
    return b


def mean_abs_prop(adj, x, K):
    """mean_k |A|^k x, k = 0..K: the layer mean's propagation with every weight taken positive."""
    a = abs(adj).astype(np.float64)
    acc, y = x.copy(), x
    for _ in range(K):
        y = a @ y
        acc = acc + y
    return acc / (K + 1)


def storage_allowance(adj, grad_final, K):
    """bf16 activation storage: what the K - 1 intermediate tables of the backward chain  h_K = Gs, h_{k-1} = Gs + A h_k
    (Gs = G / (K + 1), G = the gradient rows before the propagation's backward), each rounded to bf16, may add to every element of
    the table gradient.  bf16 keeps 8 significant bits, so rounding to nearest errs by at most 2^-8 |h_k| (the project's 2^-9 in
    DESIGN.md's adjoint row is the typical figure of an inner product, not a bound on one element).  |h_k| <= sum_{j <= K-k} |A|^j
    |Gs|, and the error of h_k reaches the result through |A|^k: 2^-8 sum_{j = k..K} |A|^j |Gs| <= 2^-8 (K + 1) M |Gs| = 2^-8 M |G|,
    M = mean_k |A|^k.  K - 1 tables: (K - 1) 2^-8 (M |G|)_i under element i, to first order in 2^-8.  [N, d] float64."""
    return (K - 1) * 2.0 ** -8 * mean_abs_prop(adj, np.abs(grad_final), K)


def cpu_trajectory(case, inp, table, mlp, batches):
    """The states the steps of a case start from: the float64 trajectory (restated gradients, restated Adam over all
    parameters), every state rounded to fp32 -> per step (table, mlp, m_table, v_table, m_mlp, v_mlp) as fp32 arrays."""
    gate = mlp is not None
    ps = [f32(table)] + ([f32(t) for t in mlp] if gate else [])
    ms, vs = [np.zeros_like(t) for t in ps], [np.zeros_like(t) for t in ps]
    states = []
    for i, batch in enumerate(batches):
        states.append(([t.copy() for t in ps], [t.copy() for t in ms], [t.copy() for t in vs]))
        r = R.step(table=ps[0], mlp=ps[1:] if gate else None, batch=batch, **inp)
        gs = [r["grad_table"]] + r["grad_mlp"]
        for j in range(len(ps)):
            p2, m2, v2 = R.adam(ps[j], ms[j], vs[j], gs[j], i + 1, LR)
            ps[j], ms[j], vs[j] = f32(p2), f32(m2), f32(v2)
    return states


_GRAPHS = {}


@pytest.fixture(scope="session")
def graph_dirs(tmp_path_factory):
    for geo in GEOMETRY:
        if geo not in _GRAPHS:
            path = str(tmp_path_factory.mktemp("gate_shapes_" + geo))
            write_graph(path, geo)
            _GRAPHS[geo] = path
    return _GRAPHS


