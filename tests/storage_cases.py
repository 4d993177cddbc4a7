"""What tests/test_storage_restatement.py (CPU), tests/test_gpu_storage_step.py and tests/test_gpu_storage_features.py (GPU) share:
the graph, the hand-set table rows, the batches, the cases and the bounds of the bf16 / fp8 default fused step, and of the fp32 /
bf16 step with layer weights or edge dropout.  Test infrastructure like
tests/storage_restatement.py, which holds the arithmetic.

BOUNDS (u = 2^-24; every bound is per element and first order in u; derivations from the kernels' code):
  stored element  A stored table is compared with float64 on the DECODED inputs the implementation itself read.  Rounding to
      nearest errs by at most half a storage ulp of the value it rounds, v = ref + e with |e| <= delta (the fp32 error before
      rounding): bf16 keeps 8 significant bits, half an ulp of v in [2^e, 2^(e+1)) is 2^(e-8) exactly (between 2^-9 |v| and
      2^-8 |v|; 2^-9 |v| itself is NOT a bound: RNE of 1 + 2^-8 errs by 2^-8, and torch's own cast exceeds it on the CPU);
      fp8 2^-4 |v| + rowmax 2^-15 (tests/test_gpu_fp8.py: 3 mantissa bits above the subnormal range, steps of scale 2^-9 <=
      rowmax 2^-15 below; a row maximum that delta moves into the next binade doubles the step, which the full-step figure
      2^-15 instead of the half step 2^-16 pays for).  So |stored - ref| <= half(|ref| + delta) + delta   (stored_bound).
  SpMM            delta of  A x: conftest.spmm_sum_bound, (2 n_i + 2) u sum_j |a_ij x_j| (covers one fp32 evaluation in any order twice
      over).  The fp8 kernels multiply the weight by the column's row scale first: a power of two, exact.
  slot row        e = ((E0 + X_1 + .. + X_{K-1}) + X_K) / (K + 1): K additions and one division of terms whose absolute sum is T:
      delta_e = ((K + 2) u T + delta_last) / (K + 1), delta_last = the SpMM bound of the in-kernel (or hub-plan) last layer, 0 with
      dense_last.
  score           x = u.p - u.n, two d-term fp32 dot products in any order and one subtraction:
      delta_x = (d + 2) u (sum |u_j p_j| + sum |u_j n_j|) + sum_j (delta_u (|p| + |n|) + |u| (delta_p + delta_n)).
  log-sigmoid     logsigmoid_f(x) = min(x, 0) - log1pf(expf(-|x|)): the library calls expf / log1pf (not the __-prefixed fast
      intrinsics) and is built without fast-math; the HIP math API gives both 1 ulp = 2 u.  z = expf(-|x|) (1 + 2u);
      log1p(z (1 + 2u)) moves by 2u z / (1 + z) <= 2u log1p(z) ... <= 2u |term|; its own ulp 2u; the subtraction u:
      delta_term = 8 u |term| + sigmoid(-x) delta_x   (d term / dx = sigmoid(-x)).
  gb              sigmoid_neg_f: expf (2u), 1 + z (u), one correctly rounded division (u); times inv_B (u):
      delta_gb = 8 u |gb| + |gb| (1 - sigmoid(-x)) delta_x.
  reg term        3 d products and their sums: (d + 3) u term + 2 sum |e| delta_e  (reg_ego: the rows are exact, delta_e = 0).
  gradient rows   slot contributions gb (p - n) + lam u, gb u + lam p, -gb u + lam n: four roundings at most of terms no larger
      than |gb ..| + |lam ..|, the propagated errors of gb and the rows, and ONE rounding to 2^-50 fixed point (2^-51).  The
      fixed-point sum over the m slots naming a row is exact (so no log2 m term: c = 4 + 2 below, the 2 for the conversion to
      fp32 and the division by K + 1, k_g32 / fold_close_rows):
      delta_G = sum_slots (4 u |contribution| + propagated) + m 2^-51;  delta_Gs = delta_G / (K + 1) + 2 u |Gs|.
  backward        launch output before storage, Gs + A h: delta = delta_Gs + (first launch: |A| delta_Gs, h = Gs) + SpMM bound of
      A h + u (|Gs| + |A| |h|) for the addition; stored_bound on top for every launch but the last; the last is read from
      Adam's first moment, g_rec = M + (M' - M) / w1, good to 2^-21 (|M| + |M'|) / w1 (tests/test_gpu_gate_shapes.py).
      reg_ego adds lam cnt E0 in the last launch: 3 u of it.
  loss_out        against the sums of the GPU's own terms: (1 + ceil(log2 B)) u sum |term| (gate_cases.step_bounds' floor; [0]
      from [1] and [2]: 2 u more).
  K = 4           end to end: the first backward table is overwritten inside the step, so g_rec is compared with the float64 chain
      WITHOUT backward storage; allowance = gate_cases.storage_allowance, (K - 1) 2^-8 (M |G|)_i for bf16, and for fp8 the
      half-ulp figure derived the same way: a table h_k errs by 2^-4 |h_k| + 2^-15 rowmax(h_k), rowmax(h_k)_i <= (sum_j |A|^j r)_i
      with r_i = max_c |Gs|_ic: (K - 1) (2^-4 M |G| + 2^-15 M r 1^T); plus the fp32 part: the chain's deltas pushed through M.

THE TWO FEATURES (FEATURE_CASES; fp32 and bf16 storage, fp8 is refused with both).  Every term again from the kernels' code:
  fp32 storage    the stored table IS the fp32 evaluation: compared with delta alone, no half-ulp term (half_ulp = 0).
  weighted slot row   triplet_body / k_triplet_dense with WTS: s = X_0 w[0]; s += w[k] X_k (k < K); e = s + w[K] X_K.  K + 1
      products and K additions, no division; a summand passes through its product's rounding and at most K additions, K + 1
      roundings, one fewer than the mean's K additions + division + the bound's spare one -- so the mean's factor K + 2 is kept
      (it pays for the products' second-order terms; an fma contraction only removes roundings).  With T_w = sum_k |w[k]| |X_k|:
      delta_e = (K + 2) u T_w + |w[K]| delta_last  (delta_last: the SpMM bound of the in-kernel / hub-plan last layer).
  weighted backward   gdiv = 1: G32 = (float)(G64 2^-50) is ONE rounding, Gs = G, delta_Gs = delta_G + u |G|.  spmm_epilogue with
      M_WTS: acc = w_in (A h); g = w_add G; y = g + acc -- two products and one addition on top of the default's terms:
      delta = |w_add| delta_Gs + u |w_add G| + |w_in| (first launch: |A| delta_Gs; SpMM bound of A h) + (first launch, the only
      one with w_in != 1: u |w_in| |A| |h|) + u (|w_add G| + |w_in| |A| |h|).  A zero weight needs no allowance: 0 G is exact
      and every term it multiplies vanishes from the bound as it does from the launch.
  dropout         drop_apply stages fl32(val fl32(1 / keep)) or 0: the restatement's matrix holds exactly these fp32 numbers, so
      the staged weight adds nothing and every bound above is taken with |A_drop| (forward, slot rows) or |A_drop^T|
      (backward) in the place of |A|: spmm_sum_bound on the masked, scaled CSR.  Dropped entries are stored as explicit zeros
      and counted in n_i (the kernel may add their exact zero products; that only loosens (2 n_i + 2) u S_i, S_i ignores them).
      Rows outside the batch's reach are rows outside the reach of the DROPPED graph's transpose: a backward launch on the
      untransposed or undropped graph writes non-zero rows there, asserted exactly zero.
  K = 4 with a feature   storage_allowance's argument with the chain's own coefficients: the stored h_{k-1} = w[k-1] G + B h_k
      (B = the backward's matrix, h_K = w[K] G; the mean: w = 1 / (K + 1)) has |h_{k-1}| <= sum_{j >= k-1} |w[j]| |B|^(j-k+1) |G| and
      reaches the result through |B|^(k-1): each of the K - 1 tables adds at most 2^-8 sum_j |w[j]| |B|^j |G|."""
import os

import numpy as np
import pytest
import torch

from conftest import EPS32, spmm_sum_bound
from gate_cases import mean_abs_prop, storage_allowance

N_USERS, M_ITEMS = 300, 600
HUB_USER, HUB_USER_DEG = 0, 520           # > 512 items: more than four 128-entry units of k_triplet, the wave order wraps
HUB_ITEM, HUB_ITEM_DEG = 0, 250
ISOLATED_ITEM = 598                       # named by test.txt only: an empty adjacency row
LR, DECAY, MODEL_SEED = 1e-3, 1e-4, 2020
BATCH_SIZES = (64, 64, 37, 1)
# hand-set table rows (on top of the N(0, 0.1) initial table)
ZERO_USER, OUTLIER_ITEM, SUBNORMAL_ITEM, TINY_USER, BIG_ITEM = 5, 7, 9, 11, 13

# (mode, d, K, dense_last, hub_nnz, reg_rows)
CASES = [("fp8", d, K, dl, -1, "propagated") for d in (64, 128, 256) for K in (1, 2, 3) for dl in (0, 1)]
CASES += [("bf16", d, K, dl, -1, "propagated") for d in (32, 64, 128, 256) for K in (1, 2, 3) for dl in (0, 1)]
CASES += [("bf16", 64, 2, 0, 100, "propagated"), ("fp8", 128, 2, 0, 100, "propagated")]          # the hub plan supplies the long rows' last layer
CASES += [("bf16", 64, 3, 0, -1, "ego"), ("fp8", 128, 2, 0, -1, "ego")]
K4_CASES = [("bf16", 128, 4, 0, -1, "propagated"), ("fp8", 128, 4, 0, -1, "propagated")]
EPOCH_CASES = [(mode, d, K, dl, -1, "propagated") for mode in ("bf16", "fp8") for d in (64, 128) for K in (2, 3) for dl in (0, 1)]
BATCH_SEED = {}                           # seed of a case's batches: 0 unless a condition of test_storage_restatement.py fails there

# ---- the two features: (mode, d, K, dense_last, hub_nnz, reg_rows, feature), feature = ("w", weight set) | ("drop", keep_prob) --
DROP_SEED = 2020                          # world's default --seed: what model.LightGCN hands to lgcn_ctx_set_dropout
_GRID = [(mode, d, K, dl) for d in (32, 64, 128, 256) for mode in ("fp32", "bf16") for K in (1, 2, 3) for dl in (0, 1)]
WEIGHT_CASES = [(mode, d, K, dl, -1, "propagated", ("w", "literal")) for mode, d, K, dl in _GRID]
WEIGHT_CASES += [("bf16", d, K, 0, -1, "propagated", ("w", name)) for d in (32, 128) for name, K in (("midzero", 3), ("last", 2), ("first", 3))]
WEIGHT_CASES += [("bf16", 64, 2, 0, 100, "propagated", ("w", "literal")), ("fp32", 256, 3, 0, 100, "propagated", ("w", "literal"))]
WEIGHT_CASES += [("bf16", 128, 3, 0, -1, "ego", ("w", "literal")), ("fp32", 32, 1, 0, -1, "ego", ("w", "literal"))]
DROP_CASES = [(mode, d, K, dl, -1, "propagated", ("drop", 0.6)) for mode, d, K, dl in _GRID]
DROP_CASES += [("bf16", 64, 2, 0, 100, "propagated", ("drop", 0.6)), ("fp32", 128, 3, 0, 100, "propagated", ("drop", 0.6))]
DROP_CASES += [("bf16", 32, 2, 0, -1, "ego", ("drop", 0.6)), ("fp32", 256, 1, 0, -1, "ego", ("drop", 0.6))]
DROP_CASES += [("bf16", 128, 2, 0, -1, "propagated", ("drop", 0.9))]
FEATURE_CASES = WEIGHT_CASES + DROP_CASES
FEATURE_K4_CASES = [("bf16", 128, 4, 0, -1, "propagated", ("w", "literal")), ("bf16", 128, 4, 0, -1, "propagated", ("drop", 0.6))]
FEATURE_EPOCH_CASES = [("bf16", d, K, dl, -1, "propagated", f) for f in (("w", "literal"), ("drop", 0.6)) for d in (32, 128) for K in (2, 3) for dl in (0, 1)]


def feature(c):
    """-> (kind, value) of a case: ("w", weight set), ("drop", keep_prob) or (None, None) for the default step."""
    return c[6] if len(c) > 6 else (None, None)


def case_weights(c):
    """The fp32 layer weights of a case (tests/test_gpu_layer_weights.py weight_set), or None."""
    kind, v = feature(c)
    if kind != "w":
        return None
    from test_gpu_layer_weights import weight_set
    return weight_set(v, c[2])


def case_keep(c):
    kind, v = feature(c)
    return float(v) if kind == "drop" else 1.0


def case_graphs(adj, c, step):
    """(forward CSR, backward CSR) of step `step` (0-based: the step counter before the step) of a case: (A_drop, A_drop^T as
    the backward launches read it) under dropout, else (A, A)."""
    from dropout_restatement import dropped_graphs
    return dropped_graphs(adj, case_keep(c), DROP_SEED, step)


def case_id(c):
    mode, d, K, dl, hub, reg = c[:6]
    kind, v = feature(c)
    feat = "" if kind is None else (f"-w_{v}" if kind == "w" else f"-drop{v}")
    return f"{mode}-d{d}-K{K}-dl{dl}" + (f"-hub{hub}" if hub > 0 else "") + ("-ego" if reg == "ego" else "") + feat


def write_graph(path, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    os.makedirs(path, exist_ok=True)
    hub_fans = set(rng.choice(np.arange(1, N_USERS - 10), size=HUB_ITEM_DEG - 1, replace=False).tolist())
    free = np.array([i for i in range(1, M_ITEMS) if i != ISOLATED_ITEM])
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(N_USERS):
            if u == HUB_USER:
                items = [HUB_ITEM] + rng.choice(free, size=HUB_USER_DEG - 1, replace=False).tolist()
            elif u >= N_USERS - 10:                                   # users of degree 1
                items = [M_ITEMS - 1] if u == N_USERS - 1 else [int(rng.choice(free))]
            else:
                items = rng.choice(free, size=int(rng.integers(2, 20)), replace=False).tolist()
                if u in hub_fans:
                    items.append(HUB_ITEM)
            f.write(f"{u} " + " ".join(map(str, sorted(items))) + "\n")
            ft.write(f"{u} {ISOLATED_ITEM if u == 0 else int(rng.integers(0, M_ITEMS))}\n")
    return path


def set_rows(table):
    """The hand-set rows, in place on an [N, d] fp32 torch table."""
    d = table.shape[1]
    with torch.no_grad():
        table[ZERO_USER] = 0.0                                        # a zero row on a connected user
        r = N_USERS + OUTLIER_ITEM                                    # one element 50 x the rest: the rest keeps one or two fp8 binades
        table[r] /= 50.0; table[r, 3] = 0.1
        r = N_USERS + SUBNORMAL_ITEM                                  # one element 2^15 x the rest: the rest IS subnormal in fp8 (below 2^-6 of
        table[r] *= 2.0 ** -15; table[r, d - 2] = -0.1                #   a scaled maximum in [64, 128))
        table[TINY_USER] *= 2.0 ** -20
        table[N_USERS + BIG_ITEM] *= 2.0 ** 6
        table[-1] = torch.linspace(-0.2, 0.2, d)                      # the last row of the table
    return table


def make_batches(case):
    rng = np.random.Generator(np.random.PCG64(1000 * BATCH_SEED.get(case_id(case), 0) + case[1] + case[2]))
    out = []
    for nb in BATCH_SIZES:
        u = rng.integers(1, N_USERS, nb); p = rng.integers(1, M_ITEMS, nb); n = rng.integers(1, M_ITEMS, nb)
        for a in (p, n):                                              # the big row propagates, no slot names it (no saturated sigmoid)
            a[(a == BIG_ITEM) | (a == ISOLATED_ITEM)] = 20
        if nb > 8:
            p[:6] = 21                                                # a row named by many slots
            n[6] = p[6]                                               # pos = neg
            u[7] = HUB_USER; u[8] = HUB_USER                          # the hub user
            p[9] = HUB_ITEM; n[10] = HUB_ITEM                         # the hub item as positive and as negative
            n[11] = ISOLATED_ITEM                                     # the isolated item as negative
            u[12] = ZERO_USER; u[13] = TINY_USER; p[14] = OUTLIER_ITEM; n[15] = SUBNORMAL_ITEM; p[16] = M_ITEMS - 1; u[17] = N_USERS - 1
        out.append((u, p, n))
    return out


def configure(pkg, case, path, batch=64):
    mode, d, K, dl, hub, reg = case[:6]
    w = pkg.world
    w.configure([])
    w.dataset = "storage_step"
    w.config.update({'lightGCN_n_layers': K, 'latent_dim_rec': d, 'bpr_batch_size': batch, 'decay': DECAY, 'lr': LR, 'act_dtype': mode,
                     'dense_last': str(dl), 'hub_nnz': hub, 'reg_rows': reg, 'checkpoint_dir': os.path.join(path, "ckpt")})
    if case_weights(case) is not None:
        w.config['layer_weights'] = "[" + ",".join(repr(float(v)) for v in case_weights(case)) + "]"
    if case_keep(case) < 1.0:
        assert w.config['seed'] == DROP_SEED
        w.config.update({'dropout': 1, 'keep_prob': case_keep(case)})
    return w


def make_model(pkg, case, path, batch=64):
    """The dataset and a fresh CPU model of a case (seed MODEL_SEED, hand-set rows in); the caller resets world's config."""
    w = configure(pkg, case, path, batch)
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(MODEL_SEED)
    m = pkg.model.LightGCN(w.config, ds)
    set_rows(m._table)
    m.train()
    return ds, m


# ---- bounds ----------------------------------------------------------------------------------------------------------------
U = EPS32


def half_ulp(ref, mode, delta=0.0):
    """Half a storage ulp of the value that is rounded, |v| <= |ref| + delta.  bf16 keeps 8 significant bits: half an ulp of v in
    [2^e, 2^(e+1)) is 2^(e-8) exactly, between 2^-9 |v| and 2^-8 |v| (2^-9 |v| itself is no bound: RNE of 1 + 2^-8 errs by 2^-8)."""
    ref = np.abs(ref) + delta
    if mode == "fp32":               # the stored table is the fp32 evaluation itself: delta alone
        return np.zeros_like(ref)
    if mode == "bf16":
        return np.where(ref > 0, 2.0 ** (np.floor(np.log2(np.maximum(ref, 1e-300))) - 8), 0.0)
    return 2.0 ** -4 * ref + ref.max(axis=1, keepdims=True) * 2.0 ** -15


def stored_bound(ref, delta, mode):
    return half_ulp(ref, mode, delta) + delta + 1e-37


def spmm_delta(adj, x):
    return spmm_sum_bound(adj.indptr, adj.data, adj.indices, x)


def np64(t):
    return t.detach().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, np.float64)


def step_deltas(adj, r, K, dense_last, reg_ego, weights=None, adj_bwd=None):
    """The fp32 error bounds of one step's quantities from its float64 restatement r (storage_restatement.step) -> dict:
    e [3, B, d], x, term, regterm, gb [B], Gs [N, d], bwd_pre {i: [N, d]}, g_final [N, d]  (module docstring).  adj: the CSR of
    the forward (A_drop under dropout), adj_bwd: of the backward (default: adj); weights: the layer weights or None."""
    rows, e, d = r["rows"], np64(r["e"]), r["e"].shape[2]
    flat = rows.reshape(-1)
    d_last = np.zeros_like(e) if dense_last else spmm_delta(adj, np64(r["last_in"]))[flat].reshape(e.shape)
    if weights is not None:
        w = [abs(float(v)) for v in weights]
        de = (K + 2) * U * np64(r["terms_abs"]) + w[K] * d_last
    else:
        de = ((K + 2) * U * np64(r["terms_abs"]) + d_last) / (K + 1)
    adj = adj if adj_bwd is None else adj_bwd               # (everything below is the backward)
    u, p, n = np.abs(e)
    du, dp, dn = de
    x, term, gb = np64(r["x"]), np64(r["term"]), np64(r["gb"])
    dx = (d + 2) * U * ((u * p).sum(1) + (u * n).sum(1)) + (du * (p + n) + u * (dp + dn)).sum(1)
    s = 1.0 / (1.0 + np.exp(x))                                       # sigmoid(-x)
    out = {"e": de, "x": dx, "term": 8 * U * np.abs(term) + s * dx + 1e-37, "gb": 8 * U * np.abs(gb) + np.abs(gb) * (1.0 - s) * dx}
    out["regterm"] = (d + 3) * U * np64(r["regterm"]) + (0.0 if reg_ego else 2.0 * (np.abs(e) * de).sum(axis=(0, 2))) + 1e-37
    lam = 0.0 if reg_ego else r["lam"]
    g, dg = np.abs(gb)[:, None], out["gb"][:, None]
    es = np64(r["e"])
    pn = np.abs(es[1] - es[2])
    dc = np.stack([dg * pn + g * (dp + dn) + lam * du + 4 * U * (g * pn + lam * u),
                   dg * u + g * du + lam * dp + 4 * U * (g * u + lam * p),
                   dg * u + g * du + lam * dn + 4 * U * (g * u + lam * n)]) + 2.0 ** -51
    dG = np.zeros(np64(r["G"]).shape)
    np.add.at(dG, flat, dc.reshape(-1, d))
    Gs = np64(r["Gs"])
    out["Gs"] = dG / (K + 1) + 2 * U * np.abs(Gs) if weights is None else dG + U * np.abs(Gs)
    aabs = abs(adj).astype(np.float64)
    out["bwd_pre"] = {}
    for i in range(K):
        h = np64(r["bwd_in"][i])
        if weights is None:
            dl = out["Gs"] + (aabs @ out["Gs"] if i == 0 else 0.0) + spmm_delta(adj, h) + U * (np.abs(Gs) + aabs @ np.abs(h))
        else:
            w_add, w_in = w[K - i - 1], (w[K] if i == 0 else 1.0)
            ah = aabs @ np.abs(h)
            dl = (w_add * out["Gs"] + U * w_add * np.abs(Gs) + w_in * ((aabs @ out["Gs"] if i == 0 else 0.0) + spmm_delta(adj, h))
                  + (U * w_in * ah if i == 0 else 0.0) + U * (w_add * np.abs(Gs) + w_in * ah))
        if i == K - 1:
            if reg_ego:
                dl = dl + 3 * U * np.abs(r["lam"] * np64(r["cnt"])[:, None] * np64(r["E0"]))
            out["g_final"] = dl
        else:
            out["bwd_pre"][i] = dl
    return out


def loss_floor(terms):
    """gate_cases.step_bounds' floor for ONE fp32 number that is a sum of n fp32 terms."""
    return (1 + int(np.ceil(np.log2(max(len(terms), 1))))) * U * float(np.abs(terms).sum()) if len(terms) > 1 else U * float(np.abs(terms).sum())


def reach(adj, rows, hops):
    """bool [N]: rows within `hops` hops of the batch rows."""
    named = np.zeros((adj.shape[0], 1))
    named[rows.reshape(-1)] = 1.0
    return mean_abs_prop(adj, named, hops)[:, 0] > 0.0


def k4_allowance(adj, G, K, mode):
    """End-to-end allowance for the backward storage of a K-layer chain (module docstring, K = 4)."""
    if mode == "bf16":
        return storage_allowance(adj, G, K)
    r = np.repeat(np.abs(G).max(axis=1, keepdims=True), G.shape[1], axis=1)
    return (K - 1) * (2.0 ** -4 * mean_abs_prop(adj, np.abs(G), K) + 2.0 ** -15 * mean_abs_prop(adj, r, K))


def feature_k4_allowance(adj_bwd, G, K, weights=None):
    """bf16 end-to-end allowance of a K-layer backward chain with layer weights (None: the mean's 1 / (K + 1)) on the backward's
    matrix (module docstring, K = 4 with a feature): (K - 1) 2^-8 sum_j |w[j]| |B|^j |G|."""
    w = [1.0 / (K + 1)] * (K + 1) if weights is None else [abs(float(v)) for v in weights]
    a = abs(adj_bwd).astype(np.float64)
    y = np.abs(G)
    acc = w[0] * y
    for j in range(1, K + 1):
        y = a @ y
        acc = acc + w[j] * y
    return (K - 1) * 2.0 ** -8 * acc


def bytes_agree(got_b, got_s, ref_b, ref_s):
    """(share of rows with the restated scale, share of equal bytes in those rows)"""
    same = got_s == ref_s
    return float(same.mean()), float((got_b[same] == ref_b[same]).mean()) if same.any() else 1.0


_GRAPH = {}


@pytest.fixture(scope="session")
def storage_graph(tmp_path_factory):
    if "path" not in _GRAPH:
        _GRAPH["path"] = write_graph(str(tmp_path_factory.mktemp("storage_step")))
    return _GRAPH["path"]
