"""float64 restatement of the fused step (train_forward, train_bpr, triplet_body / k_triplet_dense, triplet_finish,
train_backward_layer of csrc/lgcn_train.cpp and the Adam epilogue of csrc/lgcn_device.hip) with every storage point written out, and its float32 twin
(the same function with dtype = torch.float32 and the real casts).  Test infrastructure: tests/test_storage_restatement.py
pins it to the oracle, tests/test_gpu_storage_step.py judges the bf16 / fp8 kernels by it.

Storage points (Q = the rounding of the activation storage mode; `mode` is 'fp32' (identity), 'bf16' or 'fp8'):
  forward   K >= 2: layer 1 gathers Q(E0) (a conversion of its own: launch_to_bf16 / launch_to_fp8, or the Adam epilogue's
            shadow inside a multi-step call); K = 1: no shadow exists, layer 1 gathers the fp32 table whatever the mode.
            X_k = Q(A in_k), k = 1 .. fwd_layers (K with dense_last, else K - 1).  Without dense_last the last layer exists on
            the batch rows only, in fp32, gathered from X_{K-1} (from E0 when K = 1).
  slot row  e = ((E0[row] + X_1[row] + ... + X_{K-1}[row]) + X_K[row]) / (K + 1), the E0 term being the fp32 row itself.
  loss      x = e_u.e_p - e_u.e_n, term = logsigmoid(x), reg term = |e_u|^2 + |e_p|^2 + |e_n|^2 (reg_ego: of the E0 rows),
            loss_out = (bpr + decay reg, bpr = -sum term / B, reg = 0.5 sum reg term / B).
  rows      gb = -sigmoid(-x) / B, lam = decay / B (0 inside the rows with reg_ego): gb (p - n) + lam u, gb u + lam p,
            -gb u + lam n, added per table row.  reg_ego: the epilogue adds lam cnt[row] E0[row] to the final gradient.
  backward  straight-through (Q has gradient 1).  Gs = G / (K + 1) in fp32; launch k = K .. 1 computes Gs + A h with h = Gs for
            the first launch and the STORED output of the launch before it otherwise; every launch but the last stores Q(.),
            the last one feeds Adam in fp32.

The two optional axes of step() (None / absent: the default step, bit for bit what it was):
  weights   --layer_weights, fp32 w_0 .. w_K used as given: slot row e = w[0] E0[row] + sum_{k=1..K-1} w[k] X_k[row] + w[K] X_K[row]
            in that order (triplet_body / k_triplet_dense with WTS), no division by K + 1; G stays UNSCALED (gdiv = 1, Gs = G);
            backward launch i (k = K - i) computes w[k-1] G + w_in (A h), w_in = w[K] and h = G for the first launch, w_in = 1 and
            h = the stored output of the launch before it afterwards (M_WTS).  Storage points and reg_ego as above.
  dropout   A_fwd = A_drop for the forward links and the slot rows' last layer, A_bwd = A_drop^T for the backward chain; the
            entries are the fp32 values fl32(val fl32(1 / keep)) where kept, else 0 (drop_apply; exact in float64), built by
            tests/dropout_restatement.py -- the transpose explicitly, the mask is not symmetric.

Chain of custody: `custody` = {'e0s': .., 'fwd': {k: ..}, 'bwd': {i: ..}} replaces the INPUT of the following link by the given
(decoded) table wherever one is given, while the link's own output is still recorded -- every link is then restated on the
numbers the judged implementation itself stored, and no rounding flip of an earlier link travels on."""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32


# ---- the storage roundings -------------------------------------------------------------------------------------------------
def _rne_sig(x, bits):
    """x rounded to `bits` significant binary digits, ties to even (no range limits)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def bf16_round(x):
    """float64 / float32 -> the nearest bf16 value (8 significant bits; RNE), in x's dtype.  float32 goes through torch's cast."""
    if x.dtype == F32:
        return x.to(torch.bfloat16).to(F32)
    return _rne_sig(x, 8)


def fp8_parts(x):
    """The library's fp8 table of an [n, d] array, restated in x's own precision (tests/test_gpu_fp8.py quantise_rows for
    float32): scale = 2^(e - 6) for max |row| = 1.f 2^e, rows below 2^-100 -> zeros with scale 1; element = RNE(x / scale) to
    E4M3 (4 significant bits above 2^-6, steps of 2^-9 below).  -> (bytes uint8 [n, d] numpy, scale float64 [n] numpy, decoded
    tensor in x's dtype)"""
    if x.dtype == F32:
        from test_gpu_fp8 import decode, quantise_rows
        b, s = quantise_rows(x.numpy())
        return b, s.astype(np.float64), torch.from_numpy(decode(b, s))
    amax = x.abs().amax(dim=1)
    ok = amax >= 2.0 ** -100
    _, e = torch.frexp(torch.where(ok, amax, torch.ones_like(amax)))
    scale = torch.where(ok, torch.ldexp(torch.ones_like(amax), e - 1 - 6), torch.ones_like(amax))
    q = torch.where(ok[:, None], x / scale[:, None], torch.zeros_like(x))
    q = torch.where(q.abs() >= 2.0 ** -6, _rne_sig(q, 4), torch.round(q * 512.0) / 512.0)
    b = q.to(F32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()          # q is an E4M3 value: the cast is exact
    return b, scale.numpy(), q * scale[:, None]


def quantise(x, mode):
    if mode == "fp32":
        return x
    return bf16_round(x) if mode == "bf16" else fp8_parts(x)[2]


def ste(x, mode):
    """Q with gradient 1 (for autograd)."""
    return x + (quantise(x.detach(), mode) - x.detach())


# ---- the step --------------------------------------------------------------------------------------------------------------
def dense_adj(adj, dtype=F64):
    return torch.from_numpy(np.asarray(adj.todense(), np.float64)).to(dtype)


def slots(batch, n_users):
    u, p, n = (np.asarray(t, np.int64) for t in batch)
    return np.stack([u, n_users + p, n_users + n])          # [3, B] table rows


def constants(decay, B):
    """inv_B and lam as train_bpr makes them (fp32 quotients of fp32 operands): inputs of both precisions."""
    return float(np.float32(1.0) / np.float32(B)), float(np.float32(decay) / np.float32(B))


def forward(A, E0, K, mode, dense_last, rows, custody=None, q=quantise, weights=None):
    """-> dict: e0s (layer 1's input), fwd_pre / fwd {k: [N, d]} (before / after storage), last [3, B, d] (X_K on the slot rows),
    terms_abs [3, B, d] (the absolute sum of a slot row's summands, for bounds), e [3, B, d].  A is the matrix of the forward
    (A_drop under edge dropout); weights = the K + 1 fp32 layer weights as floats, or None for the mean."""
    cu = custody or {}
    fwd_layers = K if dense_last else K - 1
    out = {"fwd_pre": {}, "fwd": {}}
    out["e0s"] = q(E0, mode) if K >= 2 else E0
    prev = cu.get("e0s", out["e0s"]) if K >= 2 else E0
    used = {0: E0}
    for k in range(1, fwd_layers + 1):
        out["fwd_pre"][k] = A @ prev
        out["fwd"][k] = q(out["fwd_pre"][k], mode)
        prev = cu.get("fwd", {}).get(k, out["fwd"][k])
        used[k] = prev
    out["last_in"] = prev
    flat = rows.reshape(-1)
    last = used[K][flat] if dense_last else A[flat] @ prev
    shape = (3, rows.shape[1], E0.shape[1])
    if weights is not None:          # triplet_body / k_triplet_dense with WTS: products summed in layer order, no division
        w = [float(v) for v in weights]
        assert len(w) == K + 1
        base = w[0] * E0[flat]
        for k in range(1, K):
            base = base + w[k] * used[k][flat]
        e = base + w[K] * last
        out["last"], out["e"] = last.reshape(shape), e.reshape(shape)
        out["terms_abs"] = (sum(abs(w[k]) * used[k][flat].abs() for k in range(K)) + abs(w[K]) * last.abs()).reshape(shape)
        return out
    base = E0[flat]
    for k in range(1, K):
        base = base + used[k][flat]
    e = (base + last) / float(K + 1)
    out["last"], out["e"] = last.reshape(shape), e.reshape(shape)
    out["terms_abs"] = (sum(used[k][flat].abs() for k in range(K)) + last.abs()).reshape(shape)
    return out


def bpr(e, e0rows, n_rows, rows, K, decay, reg_ego, scaled=True):
    """triplet_loss_regs + triplet_finish on the slot rows e [3, B, d] -> dict: x, term, regterm [B], gb [B], contrib [3, B, d],
    G [N, d], Gs, cnt [N], loss_out (total, bpr, reg).  scaled = False (layer weights: gdiv = 1): Gs = G."""
    B = e.shape[1]
    inv_B, lam = constants(decay, B)
    u, p, n = e[0], e[1], e[2]
    x = (u * p).sum(1) - (u * n).sum(1)
    term = torch.nn.functional.logsigmoid(x)
    r = e0rows if reg_ego else e
    regterm = ((r[0] * r[0]).sum(1) + (r[1] * r[1]).sum(1)) + (r[2] * r[2]).sum(1)
    gb = -inv_B * torch.sigmoid(-x)
    lm = 0.0 if reg_ego else lam
    contrib = torch.stack([gb[:, None] * (p - n) + lm * u, gb[:, None] * u + lm * p, -gb[:, None] * u + lm * n])
    flat = torch.from_numpy(rows.reshape(-1))
    G = torch.zeros(n_rows, e.shape[2], dtype=e.dtype).index_add(0, flat, contrib.reshape(-1, e.shape[2]))
    cnt = torch.zeros(n_rows, dtype=e.dtype).index_add(0, flat, torch.ones(flat.numel(), dtype=e.dtype))
    bpr_l = -(term.sum() / float(B))
    reg = (0.5 * regterm.sum()) / float(B)
    return dict(x=x, term=term, regterm=regterm, gb=gb, contrib=contrib, G=G, Gs=G / float(K + 1) if scaled else G, cnt=cnt, lam=lam,
                loss_out=(bpr_l + float(np.float32(decay)) * reg, bpr_l, reg))


def backward(A, Gs, K, mode, custody=None, q=quantise, ego=None, weights=None):
    """The Horner chain.  -> dict: bwd_pre / bwd {i: [N, d]} for launch i = 0 .. K - 2 (before / after storage), g_final [N, d]
    (what Adam gets).  ego = (lam, cnt, E0) adds lam cnt[row] E0[row] in the last launch.  A is the matrix of the backward
    (A_drop^T under edge dropout).  weights: launch i (k = K - i) computes w[k-1] G + w_in (A h), w_in = w[K] for the first
    launch (h = G, unscaled) and 1 afterwards (spmm_epilogue with M_WTS)."""
    cu = (custody or {}).get("bwd", {})
    out = {"bwd_pre": {}, "bwd": {}, "bwd_in": {}}
    h = Gs
    for i in range(K):
        out["bwd_in"][i] = h
        if weights is not None:
            y = float(weights[K - i - 1]) * Gs + (float(weights[K]) * (A @ h) if i == 0 else A @ h)
        else:
            y = Gs + A @ h
        if i == K - 1:
            if ego is not None:
                y = y + (ego[0] * ego[1])[:, None] * ego[2]
            out["g_final"] = y
        else:
            out["bwd_pre"][i] = y
            out["bwd"][i] = q(y, mode)
            h = cu.get(i, out["bwd"][i])
    return out


def step(A, n_users, K, decay, table, batch, mode, dense_last=False, reg_ego=False, dtype=F64, custody=None, q=quantise, q_bwd=True,
         weights=None, A_fwd=None, A_bwd=None):
    """One fused step at the fp32 parameters `table` (numpy) -> everything the links above return, in `dtype`.  The two optional
    axes: weights = the K + 1 fp32 layer weights, used as given (--layer_weights); A_fwd / A_bwd = dense A_drop and its
    explicit transpose (--dropout: the forward links and the slot rows' last layer use A_fwd, the backward chain A_bwd; the
    mask is not symmetric).  Without them: the default step on A, every result what it was."""
    E0 = torch.from_numpy(np.asarray(table, np.float32)).to(dtype)
    A_fwd = (A if A_fwd is None else A_fwd).to(dtype)
    A_bwd = (A if A_bwd is None else A_bwd).to(dtype)
    rows = slots(batch, n_users)
    f = forward(A_fwd, E0, K, mode, dense_last, rows, custody, q, weights)
    e0rows = E0[rows.reshape(-1)].reshape(f["e"].shape)
    b = bpr(f["e"], e0rows, E0.shape[0], rows, K, decay, reg_ego, scaled=weights is None)
    w = backward(A_bwd, b["Gs"], K, mode if q_bwd else "fp32", custody, q, (b["lam"], b["cnt"], E0) if reg_ego else None, weights)
    return dict(f, **b, **w, rows=rows, E0=E0, e0rows=e0rows)


def adam(p, m, v, g, step_no, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor step in float64 on numpy arrays -> (p', m', v')."""
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step_no, 1.0 - b2 ** step_no
    return p - (lr / bc1) * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps), m2, v2
