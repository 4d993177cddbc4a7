"""The alignment-and-uniformity loss in the fused step (--loss directau; lgcn_train_step_directau, csrc/lgcn_directau.hip, DESIGN
4.26) on the GPU (-m gpu), on the graph and table of tests/storage_cases.py with the batches of tests/directau_restatement.py,
against the float64 restatement in that file.  Every step is judged from the GPU's OWN state before the step.

BOUNDS (u = 2^-24; per element; magnitudes from the restatement; computed by tests/directau_bounds.py, which follows these lines).
The forward / slot rows / sum of squares / sqrtf / division / e . inv (rho, delta_x) / score / projected row / lam e / reg term /
reg_ego / fixed point / backward / loss_out lines are those of tests/test_gpu_inbatch_scores.py (and, through it,
tests/test_gpu_inbatch.py and tests/test_gpu_softmax.py) and are not repeated: the score line is applied to x.x and y.y
(delta_s = (d + 1) u sum |x_b| |x_c| + the operand deltas), the projected-row line to W = coef k with n = min(Bp, 256).  New
(x a stored normalised row with its bound delta_x, CPT = d / min(d, 64)):
  q_b           the fp32 sum of squares of the STORED row (CPT fmaf terms in the lane, 6 additions in the tree), against 1:
                delta_q = (CPT + 7) u sum x^2 + 2 sum |x| delta_x.  This IS the unit-norm error: the kernel forms the squared
                distance as (q_b + q_c) - 2 s_bc and never assumes q = 1.
  k             D2 = (q_b + q_c) - 2 s: one addition (u (2 + delta_q_b + delta_q_c)), one fmaf (u |D2|), against 2 - 2 s:
                delta_D2 = delta_q_b + delta_q_c + u (2 + ..) + 2 delta_s + u (D2 + the former).  The product with -2 is exact.
                k = expf(-2 D2), expf to 1 ulp (2 u relative).  NOT first order (bf16 rows: delta_s is a few 1e-3):
                delta_k = k (expm1(2 delta_D2) + 2 u exp(2 delta_D2)).     k is in [e^-8, 1]: no shift, no underflow.
  Z             every pair b < c once, all terms > 0.  A term passes at most 16 * 8 = 128 additions in its lane (16 rows a
                tile, 8 tiles a part), 6 in the wave's xor tree, ceil(tiles * parts / 64) in the merge's lane-strided sum and 6
                in its tree: nZ = 140 + ceil(tiles * parts / 64) (directau_bounds.z_additions: 141 up to B = 672 = 21 tiles x 3
                parts, 142 from 22 tiles x 3 parts = 66 partials on, 148 at B = 2048 = 64 tiles x 8 parts).
                delta_Z = nZ u (Z + sum delta_k) + sum_{b<c} delta_k.  A zero row that lost its mask would add exp(-4) per pair.
  unif          logf(Z / fl(npairs)): two roundings in the argument (2 u absolute in the log), logf to 1 ulp:
                delta_unif = -log1p(-delta_Z / Z) + 2 u + 2 u |unif|;   the constant gamma (unif(X) + unif(Y)) / 2: gamma as fp32,
                one addition, one product (the half is exact): delta_cst = gamma (delta_unif_X + delta_unif_Y) / 2 + 3 u |cst|.
  coefficient   coef = 2 gamma / Z (gamma as fp32, the doubling exact, one division):
                delta_coef = coef ((delta_Z / Z) / (1 - delta_Z / Z) + 3 u);   W = coef k, one product:
                delta_W = coef delta_k + delta_coef (k + delta_k) + u (coef + delta_coef) (k + delta_k).
  alignment     |x - y|^2 from dd = x - y (delta_dd = delta_x + delta_y + u |dd|), CPT fmaf terms and the tree:
                delta_al = (CPT + 7) u sum (|dd| + delta_dd)^2 + sum (2 |dd| delta_dd + delta_dd^2);
                term = -(al + cst): delta_term = delta_al + delta_cst + u |term|; a void sample's term is -cst: delta_cst.
                Its gradient inv_u 2/B (dd - t x), t = q_x - s_xy against 1 - s_xy (s_xy the lane-group dot product: (CPT + 7) u
                sum |x| |y| + the operand deltas; delta_t = delta_q + delta_s_xy + u |t|): the product t x, the subtraction, 2/B
                (a division and a product) and the product with inv (5 u + rho):
                delta = inv (1 + rho) 2/B [ delta_dd + delta_t |x| + |t| delta_x + (5 u + rho) (|dd| + |t| |x|) ], the mirror for y.
  fixed point   (NP + 2) 2^-51 per element: NP parts of the gradient sweep, the alignment term, lam e.
Every element of every tensor is judged.  Every test prints the largest share of each bound it used (recorded in
profiles/directau/README.md).  The rows used have n2 >= 2^-60, asserted in float64 by directau_bounds.bounds."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import directau_bounds as DB
import directau_restatement as DA
import storage_cases as SC
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_gate_shapes import W1, _adam_checks
from test_gpu_inbatch import _G, _dev, _drop_matrices, _model, _same, _snapshot, _state, _uncovered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SC.U
WTS = (0.4, 0.1, 0.3, 0.2)


def _g32(gamma):
    return float(np.float32(gamma))


def _cfg(gamma, **more):
    return dict(loss='directau', au_gamma=gamma, **more)


def _judge(pkg, m, batch, K, d, mode, reg, gamma, step_no, tag, w=None, keep=None, void=()):
    """One fused step from the GPU's own state -> ({link: share of its bound}, restatement, raw outputs).  void: indices of the
    samples whose ids are bad in `batch`: their terms are -cst / 0 and the step is the restatement of the sound samples with
    B_norm = B."""
    A = _G["A"]
    ego = reg == "ego"
    B = len(batch[0])
    st = m._state(max_batch=max(B, int(m.config.get('bpr_batch_size', B))), need_ctx=True)
    lib = pkg._lib.load()
    g_ = C.c_float(-1.0)
    assert lib.lgcn_ctx_get_directau(st['ctx'], C.byref(g_)) == 0 and g_.value == np.float32(gamma)
    assert lib.lgcn_ctx_get_loss(st['ctx'], None) == pkg._lib.LOSS_DIRECTAU == 4
    assert m.adam_step == step_no - 1
    before = _state(m)
    fwd = bwd = None
    Af, Ab = A, None
    if keep is not None:
        fwd, bwd = _drop_matrices(pkg, m, keep, step_no - 1)
        Af, Ab = torch.from_numpy(fwd.toarray()), torch.from_numpy(bwd.toarray())
    neg = np.zeros(B, np.int64)                                             # accepted and ignored
    out = m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(neg)).cpu().numpy().astype(np.float64)
    after = _state(m)
    t = m._dev['terms'].cpu().numpy().astype(np.float64)
    term, regt = t[:B], t[B:2 * B]
    sound = np.ones(B, bool)
    sound[list(void)] = False
    sb = tuple(np.asarray(a_)[sound] for a_ in batch[:2])
    r = DA.step(Af, SC.N_USERS, K, SC.DECAY, _g32(gamma), before["table"], sb, ego, w, B_norm=B, A_bwd=Ab)
    bd = DB.bounds(_G["adj"], r, sb, B, K, d, mode, ego, w, _g32(gamma), fwd, bwd)
    assert np.isfinite(out).all() and np.isfinite(t[:2 * B]).all() and np.isfinite(after["M"]).all()
    share = {}
    share["term"] = float((np.abs(term[sound] - r["term"].numpy()) / bd["term"]).max())
    for v_ in void:
        assert regt[v_] == 0.0
        share["term"] = max(share["term"], abs(term[v_] + float(r["cst"])) / bd["void_term"])
    share["regterm"] = float((np.abs(regt[sound] - r["regterm"].numpy()) / bd["regterm"]).max())
    for j in range(3):
        share[f"loss{j}"] = abs(out[j] - float(r["loss_out"][j])) / bd["loss"][j]
    slack = 2.0 ** -21 * (np.abs(before["M"]) + np.abs(after["M"])) / W1
    g_rec = before["M"] + (after["M"] - before["M"]) / W1
    g_ref = r["g_final"].numpy()
    assert float(np.abs(g_rec).max()) > 0.0
    share["grad"] = float((np.abs(g_rec - g_ref) / (bd["g_final"] + slack + 1e-300)).max())
    share["adam"] = _adam_checks((tag, "table"), before["table"], before["M"], before["V"], after["table"], after["M"], after["V"],
                                 g_rec, slack, step_no, False)
    rows_ = np.unique(np.concatenate([sb[0], SC.N_USERS + sb[1]]))
    tight = float(np.median(bd["g_final"][rows_].max(1) / (np.abs(g_ref[rows_]).max(1) + 1e-300)))
    print(f"[directau] {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items())
          + f" | rho_inv {bd['rho']:.2e} dZ/Z {bd['relZ'][0]:.2e} {bd['relZ'][1]:.2e} bound/|g| median {tight:.2e}")
    return share, r, (term, regt, g_rec, slack, bd, out)


def _run(pkg, path, mode, d, K, B, gamma, reg="propagated", w=None, keep=None, batches=None, steps=2):
    try:
        cfg = _cfg(gamma)
        if w is not None:
            cfg['layer_weights'] = str(list(w))
        if keep is not None:
            cfg.update({'dropout': 1, 'keep_prob': keep, 'seed': 2020})
        _, m = _model(pkg, path, mode, d, K, reg, dl=0, batch=B, **cfg)      # --dense_last 0: the model must force the dense last layer
        top, bad = {}, []
        for i, batch in enumerate(batches or DA.make_batches(B, steps, seed=d + K)):
            tag = f"{mode} d{d} K{K} gamma{gamma} {reg}" + (" wts" if w is not None else "") + (f" keep{keep}" if keep else "") + f" step {i + 1} B={len(batch[0])}"
            share = _judge(pkg, m, batch, K, d, mode, reg, gamma, i + 1, tag, w=w, keep=keep)[0]
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        assert m._dev['dense_last'] is True
        print(f"[directau] {mode} d{d} K{K} B{B} gamma{gamma} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


# ---- 1. steps against the float64 restatement --------------------------------------------------------------------------------
_BS, _DS, _KS, _MS = (1, 2, 33, 64, 257), (32, 64, 128, 256), (1, 3), ("fp32", "bf16")
# Not the full product: every value of every axis meets at least two values of each other axis (checked below).  B = 1: no pair;
# 2: one pair; 33: one full tile and one row; 64: full tiles only; 257: one row past a 256-row part of the sweep, so the normaliser
# has two parts to merge.  d = 32, 64: the register form (IB_REG_D), one / two column blocks; 128, 256: streamed operands, one / two
# workgroups per owned tile.  reg_rows both ways and layer weights on and off at d = 64.
_CASES = [
    (1, 64, 1, 'fp32', 'propagated', False),
    (1, 256, 3, 'bf16', 'ego', False),
    (1, 32, 3, 'fp32', 'propagated', False),
    (2, 32, 3, 'bf16', 'ego', False),
    (2, 128, 1, 'fp32', 'propagated', False),
    (2, 64, 1, 'bf16', 'ego', True),
    (33, 64, 3, 'bf16', 'ego', False),
    (33, 32, 1, 'bf16', 'propagated', False),
    (33, 256, 1, 'fp32', 'propagated', False),
    (33, 128, 3, 'fp32', 'ego', False),
    (64, 128, 3, 'bf16', 'ego', False),
    (64, 64, 3, 'fp32', 'propagated', True),
    (64, 32, 1, 'fp32', 'ego', False),
    (64, 256, 1, 'bf16', 'propagated', False),
    (257, 64, 3, 'fp32', 'ego', True),
    (257, 64, 1, 'bf16', 'propagated', False),
    (257, 128, 1, 'bf16', 'ego', False),
    (257, 256, 3, 'bf16', 'propagated', False),
    (257, 32, 1, 'fp32', 'ego', False),
]
assert not _uncovered([c[:4] for c in _CASES]), _uncovered([c[:4] for c in _CASES])
assert all({c[a] for c in _CASES} == set(ax) for a, ax in enumerate((_BS, _DS, _KS, _MS)))
assert {(c[4], c[5]) for c in _CASES if c[1] == 64} == {(r_, w_) for r_ in ("propagated", "ego") for w_ in (False, True)}


@pytest.mark.parametrize("B,d,K,mode,reg,wts", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}{'-wts' if c[5] else ''}") for c in _CASES])
def test_steps_equal_the_restatement(pkg, storage_graph, B, d, K, mode, reg, wts):
    """Loss slots, per-sample terms, the gradient recovered from Adam's first moment, V and P (Adam itself), G64 zero afterwards:
    each within the bound derived in the module docstring, over two consecutive batches of B samples at gamma = 1."""
    _run(pkg, storage_graph, mode, d, K, B, 1.0, reg, w=WTS[:K + 1] if wts else None)


# ---- 1b. the batch sizes the loss is trained and timed at ----------------------------------------------------------------------
# DA.LARGE_BATCH_SIZES.  k_directau_merge adds n = tiles x parts partials per side in a lane-strided loop over 64 lanes: up
# to 21 tiles (B <= 672) n <= 63 and the loop body runs at most once per lane.  B = 705: n = 69 (the last tile holds one live row); B = 736: the
# same count with full tiles; B = 2048 (the default --bpr_batch): n = 512, eight per lane.  From three parts on the symmetric
# sweep also has workgroups whose whole part lies below the owner tile in the MIDDLE of the sweep (DA.skipped_parts), and the
# blockIdx.y extent of k_directau_norm / k_directau_grad and part[(side * NP + by) * nT + bx] run beyond by = 1.  The bounds are
# those of the module docstring, unchanged: nZ = directau_bounds.z_additions(B) counts the merge's additions, NP and n = min(Bp,
# 256) are functions of B, c(B) the loss reduction's.  d = 256 stays at B = 736 (the float64 restatement costs B^2 d and decides
# the time of a case); two steps per case.
_LARGE_CASES = [
    (705, 32, 1, 'fp32', 'ego', False),
    (705, 128, 3, 'bf16', 'propagated', False),
    (736, 256, 1, 'bf16', 'ego', False),
    (736, 64, 3, 'fp32', 'propagated', True),
    (736, 256, 3, 'fp32', 'propagated', False),
    (2048, 64, 1, 'bf16', 'propagated', False),
    (2048, 128, 3, 'fp32', 'ego', False),
    (2048, 32, 3, 'bf16', 'ego', False),
]
assert {c[0] for c in _LARGE_CASES} == set(DA.LARGE_BATCH_SIZES)
assert all(DA.partials(c[0]) > 64 for c in _LARGE_CASES) and DA.partials(672) == 63 and DA.partials(705) == DA.partials(736) == 69
assert DA.partials(2048) == 512 and max(DA.partials(c[0]) for c in _CASES) == 18
assert {DB.z_additions(B) for B in DA.LARGE_BATCH_SIZES} == {142, 148} and DB.z_additions(672) == 141 and DB.z_additions(673) == 142
assert {DB.parts(c[0]) for c in _LARGE_CASES} == {3, 8} and all(DA.skipped_parts(c[0]) for c in _LARGE_CASES) and not DA.skipped_parts(257)
assert all(sum(c[1] == d_ for c in _LARGE_CASES) >= 2 for d_ in _DS) and {c[2] for c in _LARGE_CASES} == set(_KS)
assert all({c[3] for c in _LARGE_CASES if ok(c[1])} == set(_MS) for ok in (lambda d_: d_ <= 64, lambda d_: d_ >= 128))
assert {c[4] for c in _LARGE_CASES} == {"propagated", "ego"} and all(c[0] <= 736 for c in _LARGE_CASES if c[1] == 256)
for _c_ in _LARGE_CASES:
    for _u, _p in DA.make_batches(_c_[0], 2, seed=_c_[1] + _c_[2]):
        assert _u[-1] in _u[:256] and _p[-1] in _p[:256]              # across parts: rows 0..255 / the last part


@pytest.mark.parametrize("B,d,K,mode,reg,wts", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}{'-wts' if c[5] else ''}") for c in _LARGE_CASES])
def test_steps_equal_the_restatement_at_the_training_batch_sizes(pkg, storage_graph, B, d, K, mode, reg, wts):
    """Section 1 at B = 705, 736 and 2048: the same links within the same derived bounds, over two consecutive batches that repeat
    a user and an item across parts.  The Z / unif / coefficient lines are the ones a merge that dropped partials would miss."""
    _run(pkg, storage_graph, mode, d, K, B, 1.0, reg, w=WTS[:K + 1] if wts else None)


def test_gamma_zero_and_another_gamma(pkg, storage_graph):
    """gamma = 0: the alignment loss alone (no coefficient leaves, the gradient launch adds nothing); gamma = 0.3: not the default."""
    _run(pkg, storage_graph, "fp32", 64, 3, 33, 0.0, steps=1)
    _run(pkg, storage_graph, "bf16", 128, 1, 64, 0.3, steps=1)


# ---- 2. masks, voids, duplicates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, 7])
def test_void_samples_and_padding_are_masked(pkg, storage_graph, B):
    """A void sample in the first tile and one in the last (B = 33: rows 0 and 32; B = 7: rows 0 and 6, beside 25 padding rows): err
    is set, they are part of no pair and of no alignment term, the divisors stay B and B (B - 1) / 2.  One zero row that lost its
    mask would add exp(-4) to Z per sound row: shown, in float64 on these inputs, to be more than 10 times the bound of Z."""
    try:
        d, K = 64, 1
        u, p = DA.make_batch(B, seed=5)
        u, p = u.copy(), p.copy()
        void = (0, B - 1)
        u[0] = SC.N_USERS + 3; p[B - 1] = -2
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(1.0))
        share, r, (_, _, _, _, bd, _) = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", 1.0, 1, f"void B={B}", void=void)
        assert all(v <= 1.0 for v in share.values()), share
        lost = (B - 2) * np.exp(-4.0)
        assert lost > 10 * bd["dZ"][0] and lost > 10 * bd["dZ"][1], (lost, bd["dZ"])
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


def test_void_samples_in_the_last_part(pkg, storage_graph):
    """test_void_samples_and_padding_are_masked at B = 705 (three parts, 69 partials): a void sample in row 0, one in part 1 (row
    300) and the only live row of the last tile (704), beside its 31 padding rows.  The bound of Z grows with the pair count, one
    lost row's exp(-4) per sound row only with B: here it is asserted to exceed TWICE the bound, which is what it takes for a
    result that is off by it to lie outside the bound whatever the rounding (|error| <= bound)."""
    try:
        d, K, B = 64, 1, DA.MERGE_B
        u, p = DA.make_batch(B, seed=5)
        u, p = u.copy(), p.copy()
        void = (0, 300, B - 1)
        u[0] = SC.N_USERS + 3; p[300] = SC.M_ITEMS; p[B - 1] = -2
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(1.0))
        share, r, (_, _, _, _, bd, _) = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", 1.0, 1, f"void B={B}", void=void)
        assert all(v <= 1.0 for v in share.values()), share
        lost = (B - 3) * np.exp(-4.0)
        print(f"[directau] void B={B}: a lost mask adds {lost:.3g} to Z, the bounds of Z are {bd['dZ'][0]:.3g} / {bd['dZ'][1]:.3g}")
        assert lost > 2 * bd["dZ"][0] and lost > 2 * bd["dZ"][1], (lost, bd["dZ"])
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


def test_one_sound_sample_among_void_ones(pkg, storage_graph):
    """Five samples, four of them void: no pair, so both unif are exactly 0, the constant is exactly 0 (the void samples' terms are
    -0 / 0), the loss is the one alignment term over B = 5 and only the alignment gradient and the regulariser move rows."""
    try:
        d, K, B = 64, 3, 5
        u, p = DA.make_batch(B, seed=8)
        u, p = u.copy(), p.copy()
        void = (0, 1, 3, 4)
        u[0] = -1; p[1] = SC.M_ITEMS; u[3] = SC.N_USERS; p[4] = -7
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(1.0))
        share, r, (term, _, _, _, _, out) = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", 1.0, 1, "one sound of five", void=void)
        assert all(v <= 1.0 for v in share.values()), share
        assert float(r["cst"]) == 0.0 and all(term[v_] == 0.0 for v_ in void) and float(r["gu_u"].abs().max()) == 0.0
        assert float(r["loss_out"][1]) == float(r["al"][0]) / B and out[1] > 0.0
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


def test_one_user_five_times(pkg, storage_graph):
    """One user in five samples of 33: ten pairs of distance zero on the user side (k = 1 up to rounding).  Within the bounds,
    finite."""
    u, p = DA.make_batch(33, seed=2)
    u = u.copy()
    u[[1, 9, 17, 30]] = u[0]
    assert int((u == u[0]).sum()) == 5
    _run(pkg, storage_graph, "fp32", 64, 3, 33, 1.0, batches=[(u, p)])
    _run(pkg, storage_graph, "bf16", 128, 1, 33, 1.0, batches=[(u, p)])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,d", [("fp32", 257, 64), ("bf16", 100, 256)])
def test_the_same_step_twice_is_bitwise_the_same(pkg, storage_graph, mode, B, d):
    try:
        res = []
        for _ in range(2):
            _, m = _model(pkg, storage_graph, mode, d, 3, batch=B, **_cfg(1.0))
            outs = [m.fused_step(_dev(u), _dev(p), _dev(u)).clone() for u, p in DA.make_batches(B, 2, seed=9)]
            m.check_device_errors()
            res.append(outs + [m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone(), m._dev['terms'].clone()])
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("mode,K,T", [("fp32", 1, 165), ("bf16", 3, 165), ("fp32", 3, 65)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K, T):
    """lgcn_train_epoch_directau over T = 165 (batches of 64, 64, 37) and T = 65 (64, 1: a last batch with no pair) against the loop
    of lgcn_train_step_directau: loss rows, table, both Adam moments bit for bit."""
    try:
        B, d = 64, 64
        u, p = DA.make_batch(T, seed=1)
        _, a = _model(pkg, storage_graph, mode, d, K, **_cfg(1.0))
        want = a.fused_epoch(_dev(u), _dev(p), _dev(u), B)
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, **_cfg(1.0))
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(u[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        n = (T + B - 1) // B
        assert a.adam_step == b.adam_step == n and want.shape == (n, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-4                 # (it trained)
    finally:
        pkg.world.configure([])


# ---- 4. lifecycle and refusals -----------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(pkg, storage_graph):
    try:
        L = pkg._lib
        lib = L.load()
        B = 8
        u = _dev(np.arange(B) + 20); p = _dev(np.arange(B) + 30); n = _dev(np.arange(B) + 31)
        u64, p64, n64 = (t.long() for t in (u, p, n))
        scratch = torch.full((3 * 64,), -5, dtype=torch.int32, device=DEV)
        loss = torch.full((6,), -7.0, dtype=torch.float32, device=DEV)
        stream = L.current_stream()
        # (a) while directau is set, every other training entry point
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, **_cfg(0.5))
        st = m._state(max_batch=64, need_ctx=True)
        ctx = st['ctx']
        before = _snapshot(lib, m, st)
        calls = {
            "lgcn_train_step": lambda: lib.lgcn_train_step(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), stream),
            "lgcn_train_step_i64": lambda: lib.lgcn_train_step_i64(ctx, L.tp(u64), L.tp(p64), L.tp(n64), B, L.tp(scratch), L.tp(loss), stream),
            "lgcn_train_epoch": lambda: lib.lgcn_train_epoch(ctx, L.tp(u), L.tp(p), L.tp(n), B, B, L.tp(loss), stream),
            "lgcn_train_step_multi": lambda: lib.lgcn_train_step_multi(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, B, L.tp(loss), stream),
            "lgcn_train_epoch_multi": lambda: lib.lgcn_train_epoch_multi(ctx, L.tp(u), L.tp(p), L.tp(n), 1, B, B, L.tp(loss), stream),
            "lgcn_train_step_inbatch": lambda: lib.lgcn_train_step_inbatch(ctx, L.tp(u), L.tp(p), B, L.tp(loss), stream),
            "lgcn_train_epoch_inbatch": lambda: lib.lgcn_train_epoch_inbatch(ctx, L.tp(u), L.tp(p), B, B, L.tp(loss), stream),
            "lgcn_train_step_inbatch_mix": lambda: lib.lgcn_train_step_inbatch_mix(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, B, L.tp(loss), stream),
            "lgcn_train_epoch_inbatch_mix": lambda: lib.lgcn_train_epoch_inbatch_mix(ctx, L.tp(u), L.tp(p), L.tp(n), 1, B, B, L.tp(loss), stream),
            "lgcn_train_step_dp_part1": lambda: lib.lgcn_train_step_dp_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, stream),
            "lgcn_train_step_dp_dense_part1": lambda: lib.lgcn_train_step_dp_dense_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, stream),
            "lgcn_train_step_dp_part2": lambda: lib.lgcn_train_step_dp_part2(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, None, L.tp(loss), stream),
            "lgcn_train_step_cols_part1": lambda: lib.lgcn_train_step_cols_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, None, stream),
            "lgcn_train_step_cols_part2": lambda: lib.lgcn_train_step_cols_part2(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), stream),
            "lgcn_rs_phase": lambda: lib.lgcn_rs_phase(ctx, 0, 1, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, None, L.tp(loss), stream),
            "lgcn_train_epoch_dp": lambda: lib.lgcn_train_epoch_dp(ctx, None, L.tp(u), L.tp(p), L.tp(n), B, B, 0, None, None, L.tp(loss), stream),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "directau" in msg and name in msg, (name, rc, msg)
        # (b) the new entry points: B out of range, null pointers
        for name, call in {
            "B=0": lambda: lib.lgcn_train_step_directau(ctx, L.tp(u), L.tp(p), 0, L.tp(loss), stream),
            "B>max": lambda: lib.lgcn_train_step_directau(ctx, L.tp(u), L.tp(p), 65, L.tp(loss), stream),
            "null users": lambda: lib.lgcn_train_step_directau(ctx, None, L.tp(p), B, L.tp(loss), stream),
            "null pos": lambda: lib.lgcn_train_step_directau(ctx, L.tp(u), None, B, L.tp(loss), stream),
            "null loss": lambda: lib.lgcn_train_step_directau(ctx, L.tp(u), L.tp(p), B, None, stream),
            "epoch B>max": lambda: lib.lgcn_train_epoch_directau(ctx, L.tp(u), L.tp(p), B, 65, L.tp(loss), stream),
            "epoch null": lambda: lib.lgcn_train_epoch_directau(ctx, L.tp(u), None, B, 4, L.tp(loss), stream),
        }.items():
            rc = call()
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "directau" in msg, (name, rc, msg)
        # (c) a gamma that is none; lgcn_ctx_set_loss keeps refusing every kind other than 0, 1, 2 and names the setter for 4
        for bad in (float("nan"), float("inf"), -1.0):
            rc = lib.lgcn_ctx_set_directau(ctx, bad)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "directau" in msg and "gamma" in msg, (bad, rc, msg)
        for kind in (4, 3, 7):
            rc = lib.lgcn_ctx_set_loss(ctx, kind, 1.0)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and ("lgcn_ctx_set_directau" in msg if kind == 4 else "unknown loss kind" in msg), (kind, rc, msg)
        g_ = C.c_float(0.0)
        assert lib.lgcn_ctx_get_directau(ctx, C.byref(g_)) == 0 and g_.value == 0.5
        assert lib.lgcn_ctx_get_loss(ctx, None) == L.LOSS_DIRECTAU
        torch.cuda.synchronize()
        _same(before, _snapshot(lib, m, st))
        assert bool((loss == -7.0).all()) and bool((scratch == -5).all())
        # ... and the same context takes a sound call afterwards
        bu, bp = DA.make_batch(64)
        out = m.fused_step(_dev(bu), _dev(bp), _dev(bu))
        m.check_device_errors()
        assert bool(torch.isfinite(out).all()) and m.adam_step == 1
        # (d) the new entry points on a context whose loss is not set (bpr, softmax, inbatch)
        for cfg in ({}, {'loss': 'softmax', 'softmax_temp': 0.5}, {'loss': 'inbatch', 'softmax_temp': 0.5}):
            _, mo = _model(pkg, storage_graph, "fp32", 64, 2, **cfg)
            so = mo._state(max_batch=64, need_ctx=True)
            b0 = _snapshot(lib, mo, so)
            for name, call in (("lgcn_train_step_directau", lambda: lib.lgcn_train_step_directau(so['ctx'], L.tp(u), L.tp(p), B, L.tp(loss), stream)),
                               ("lgcn_train_epoch_directau", lambda: lib.lgcn_train_epoch_directau(so['ctx'], L.tp(u), L.tp(p), B, 4, L.tp(loss), stream))):
                rc = call()
                msg = lib.lgcn_last_error().decode()
                assert rc == 3 and "directau" in msg and name in msg, (name, rc, msg)
            assert lib.lgcn_ctx_get_directau(so['ctx'], C.byref(g_)) == 3 and g_.value == 0.5
            torch.cuda.synchronize()
            _same(b0, _snapshot(lib, mo, so))
        assert bool((loss == -7.0).all())
        # (e) contexts that cannot run it: fp8 storage, dense_last = 0, hard negatives set, mixed negatives set
        for cfg, mode, dl, word in (({}, "fp8", 1, "FP8"), ({}, "fp32", 0, "dense_last"),
                                    ({'neg_ratio': 4, 'hard_neg': 2}, "fp32", 1, "hard negatives"),
                                    ({'loss': 'inbatch', 'softmax_temp': 0.5, 'inbatch_mix': 1, 'neg_ratio': 2}, "fp32", 1, "mixed negatives")):
            _, mo = _model(pkg, storage_graph, mode, 64, 2, dl=dl, **cfg)
            so = mo._state(max_batch=64, need_ctx=True)
            kind0 = lib.lgcn_ctx_get_loss(so['ctx'], None)
            b0 = _snapshot(lib, mo, so)
            rc = lib.lgcn_ctx_set_directau(so['ctx'], 1.0)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "directau" in msg and word in msg, (cfg, mode, dl, rc, msg)
            assert lib.lgcn_ctx_get_loss(so['ctx'], None) == kind0
            _same(b0, _snapshot(lib, mo, so))
    finally:
        pkg.world.configure([])


def test_bpr_and_directau_again_is_a_fresh_context(pkg, storage_graph):
    """set directau -> set BPR (a three-slot step on it is the step of a context never told) -> set directau again: from equal
    tables the step has the bits of a fresh directau context."""
    try:
        L = pkg._lib
        lib = L.load()
        d, K, B = 64, 2, 64
        u, p = DA.make_batch(B, seed=3)
        n = (p + 1) % SC.M_ITEMS
        _, ma = _model(pkg, storage_graph, "fp32", d, K, **_cfg(0.7))
        sa = ma._state(max_batch=B, need_ctx=True)
        _, mb = _model(pkg, storage_graph, "fp32", d, K)
        mb._state(max_batch=B, need_ctx=True)
        L.check(lib.lgcn_ctx_set_loss(sa['ctx'], L.LOSS_BPR, float("nan")), "set_loss")
        assert lib.lgcn_ctx_get_loss(sa['ctx'], None) == L.LOSS_BPR and lib.lgcn_ctx_get_directau(sa['ctx'], None) == 3
        loss = torch.zeros(3, dtype=torch.float32, device=DEV)
        du_, dp_, dn_ = _dev(u), _dev(p), _dev(n)                             # (held: the launches read them after the call returns)
        L.check(lib.lgcn_train_step(sa['ctx'], L.tp(du_), L.tp(dp_), L.tp(dn_), B, L.tp(loss), L.current_stream()), "bpr step")
        ob = mb.fused_step(du_, dp_, dn_)
        torch.cuda.synchronize()
        assert torch.equal(loss, ob) and torch.equal(ma._table, mb._table) and torch.equal(sa['adam_m'], mb._dev['adam_m'])
        L.check(lib.lgcn_ctx_set_directau(sa['ctx'], 0.7), "set_directau")
        # a fresh directau context from the same state
        _, mc = _model(pkg, storage_graph, "fp32", d, K, **_cfg(0.7))
        sc = mc._state(max_batch=B, need_ctx=True)
        mc._table.data.copy_(ma._table.data)
        for key in ('adam_m', 'adam_v'):
            sc[key].copy_(sa[key])
        lib.lgcn_ctx_set_step(sc['ctx'], 1)
        o1 = ma.fused_step(_dev(u), _dev(p), _dev(n)).clone()
        o2 = mc.fused_step(_dev(u), _dev(p), _dev(n)).clone()
        ma.check_device_errors(); mc.check_device_errors()
        assert torch.equal(o1, o2) and torch.equal(ma._table, mc._table)
        assert torch.equal(sa['adam_m'], sc['adam_m']) and torch.equal(sa['adam_v'], sc['adam_v'])
    finally:
        pkg.world.configure([])


# ---- 5. through the module surface -------------------------------------------------------------------------------------------
def test_module_surface_agrees_with_the_c_entry_points(pkg, storage_graph):
    """fused_step / BPRLoss.stageOne against lgcn_train_step_directau and fused_epoch against lgcn_train_epoch_directau, from equal
    fresh models: the same bits."""
    try:
        L = pkg._lib
        lib = L.load()
        d, K, B, T = 64, 2, 64, 165
        u, p = DA.make_batch(T, seed=4)
        du_, dp_ = _dev(u), _dev(p)
        # the C entry points
        _, mc = _model(pkg, storage_graph, "bf16", d, K, **_cfg(1.0))
        sc = mc._state(max_batch=B, need_ctx=True)
        l1 = torch.zeros(3, dtype=torch.float32, device=DEV)
        L.check(lib.lgcn_train_step_directau(sc['ctx'], L.tp(du_), L.tp(dp_), B, L.tp(l1), L.current_stream()), "step")
        le = torch.zeros(9, dtype=torch.float32, device=DEV)
        L.check(lib.lgcn_train_epoch_directau(sc['ctx'], L.tp(du_), L.tp(dp_), T, B, L.tp(le), L.current_stream()), "epoch")
        torch.cuda.synchronize()
        # the module
        _, mm = _model(pkg, storage_graph, "bf16", d, K, **_cfg(1.0))
        o1 = mm.fused_step(du_[:B], dp_[:B], du_[:B]).clone()
        oe = mm.fused_epoch(du_, dp_, du_, B).clone()
        mm.check_device_errors()
        assert torch.equal(o1, l1) and torch.equal(oe.reshape(-1), le) and torch.equal(mm._table, mc._table)
        assert mm.adam_step == 4 == int(lib.lgcn_ctx_get_step(sc['ctx']))
        # stageOne: the same step, its total as a float
        _, ms = _model(pkg, storage_graph, "bf16", d, K, **_cfg(1.0))
        bpr = pkg.utils.BPRLoss(ms, pkg.world.config)
        got = bpr.stageOne(du_[:B], dp_[:B], du_[:B])
        assert got == float(l1[0]) and ms.adam_step == 1
        # the autograd statement means the same thing (fp32 tables on the device, 1e-5 of a loss of order 1)
        _, mg = _model(pkg, storage_graph, "fp32", d, K, **_cfg(1.0))
        mg2 = _model(pkg, storage_graph, "fp32", d, K, **_cfg(1.0))[1]
        with torch.no_grad():
            au, rg = mg.bpr_loss(du_[:B].long(), dp_[:B].long(), du_[:B].long())
        o = mg2.fused_step(du_[:B], dp_[:B], du_[:B])
        assert abs(float(au) - float(o[1])) < 1e-5 and abs(float(rg) - float(o[2])) < 1e-5
    finally:
        pkg.world.configure([])


def test_checkpoint_and_resume_round_trip(pkg, storage_graph, tmp_path):
    """2 steps, save, load into a fresh model, 2 more steps: the bits of 4 steps in one run."""
    try:
        d, K, B = 64, 2, 64
        batches = [tuple(_dev(a) for a in (u, p, u)) for u, p in DA.make_batches(B, 4, seed=6)]

        def fresh():
            _, m = _model(pkg, storage_graph, "bf16", d, K, **_cfg(1.0))
            return m, pkg.utils.BPRLoss(m, pkg.world.config)
        ma, bpra = fresh()
        la = [bpra.stageOne(*b) for b in batches]
        md, bprd = fresh()
        ld = [bprd.stageOne(*b) for b in batches[:2]]
        ckpt = os.path.join(str(tmp_path), "last.pth.tar")
        torch.save({'model_state': md.state_dict(), 'optimizer_state': bprd.opt.state_dict()}, ckpt)
        sd = torch.load(ckpt, weights_only=True)
        me, bpre = fresh()
        me.load_state_dict(sd['model_state'])
        bpre.opt.load_state_dict(sd['optimizer_state'])
        assert me.adam_step == 2
        le = [bpre.stageOne(*b) for b in batches[2:]]
        assert ld + le == la and torch.equal(me._table, ma._table)
        for m in (ma, md, me):
            m.check_device_errors()
    finally:
        pkg.world.configure([])


def test_steps_with_edge_dropout(pkg, storage_graph):
    """--dropout 1 --keepprob 0.6: the forward and the backward run on the step's dropped graph, the loss launches are unchanged."""
    _run(pkg, storage_graph, "fp32", 64, 3, 33, 1.0, keep=0.6)
