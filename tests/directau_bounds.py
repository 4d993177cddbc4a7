"""The per-element bounds of the fused step under --loss directau from a float64 restatement
(tests/directau_restatement.py): the BOUNDS docstring of tests/test_gpu_directau.py line by line, in the manner of _bounds of
tests/test_gpu_inbatch_scores.py.  No device: tests/test_directau_host.py uses the Z line to show that a lost mask lies far outside
it; tests/test_gpu_directau.py judges the device with all of it.  Nothing here is fitted to what a kernel produced."""
import numpy as np

import inbatch_restatement as IB
import multineg_restatement as MN
import storage_cases as SC
from conftest import spmm_sum_bound

U = SC.U
MIN_N2 = 2.0 ** -60


def parts(B):
    return (((B + 31) // 32) + 7) // 8


def c_loss(n):
    return int(np.ceil(n / 64.0)) + 8


def z_additions(B):
    """Additions a term of Z passes through: 16 rows x 8 tiles in the lane, 6 in the wave's tree, the lane-strided sum of the
    merge over the (tile, part) partials and its 6-level tree."""
    nT = (B + 31) // 32
    return 128 + 6 + int(np.ceil(nT * parts(B) / 64.0)) + 6


def bounds(adj, r, batch, B, K, d, mode, ego, w, gamma, fwd=None, bwd=None):
    """-> dict: term [nb], void_term (the bound of a void sample's term -cst), regterm [nb], loss (3), g_final [N, d], rho (largest
    relative bound of an inv), relZ (x, y), dZ (x, y).  fwd / bwd: scipy CSR of the forward / backward matrix (default A_hat)."""
    extra = 2 if fwd is None else 4
    fwd = adj.astype(np.float64) if fwd is None else fwd
    bwd = fwd if bwd is None else bwd
    af, ab = abs(fwd).tocsr(), abs(bwd).tocsr()
    wk = MN.layer_weights(K, w)
    E0 = r["E0"].numpy()
    # ---- forward tables and slot rows (tests/test_gpu_softmax.py)
    X = E0
    T = abs(wk[0]) * np.abs(E0)
    dX = SC.stored_bound(E0, 0.0, "bf16") if (mode == "bf16" and K >= 2) else np.zeros_like(E0)
    dE = np.zeros_like(E0)
    for k in range(1, K + 1):
        pre = af @ dX + spmm_sum_bound(af.indptr, af.data, af.indices, np.abs(X) + dX, extra_terms=extra)
        X = fwd @ X
        dX = SC.stored_bound(X, pre, "bf16") if mode == "bf16" else pre
        T = T + abs(wk[k]) * np.abs(X)
        dE = dE + abs(wk[k]) * dX
    dE = dE + ((K + 2) if w is None else 2 * (K + 2)) * U * T
    T = T + dE
    u_, p_ = IB.as_samples(batch)
    nb = len(u_)
    ui, pi = u_, SC.N_USERS + p_
    au, ap, du, dp = T[ui], T[pi], dE[ui], dE[pi]
    NP = parts(B)
    CPT = d // min(d, 64)
    gamma = float(gamma)

    # ---- the normalised rows (the cosine lines of tests/test_gpu_inbatch_scores.py)
    def hat(a, de, inv, eh):
        n2 = 1.0 / inv ** 2
        assert (inv > 0).all() and (n2 >= MIN_N2).all()
        dn2 = (CPT + 7) * U * (a * a).sum(1) + (2 * a * de).sum(1) + d * 2.0 ** -149
        eps = dn2 / n2
        assert (eps < 0.25).all(), float(eps.max())
        rho = 0.5 * eps * (1.0 - eps) ** -1.5 + 2 * U
        dh = np.abs(eh) * (rho + U)[:, None] + de * (inv * (1 + rho))[:, None]
        return np.abs(eh) + dh, dh, rho, inv * (1 + rho)
    x, y = r["x"].numpy(), r["y"].numpy()
    hx, dhx, rho_u, inv_u = hat(au, du, r["inv_u"].numpy(), x)
    hy, dhy, rho_p, inv_p = hat(ap, dp, r["inv_p"].numpy(), y)
    n_chain = min(((B + 31) // 32) * 32, IB.PART_ROWS)
    nZ = z_additions(B)

    # ---- one side of the uniformity term: q, s, k, Z, unif, the coefficient, W, t and the projected rows
    def side(xs, h, dh, kk, Wm, Z, unif, inv, rho_o):
        zero = np.zeros_like(h)
        if nb < 2 or Z == 0.0:
            return dict(dunif=0.0, relZ=0.0, dZ=0.0, off=zero)
        dq = (CPT + 7) * U * (h * h).sum(1) + 2 * (h * dh).sum(1)
        Sabs = h @ h.T
        ds = (d + 1) * U * Sabs + dh @ h.T + h @ dh.T
        s = xs @ xs.T
        d2 = np.maximum(2.0 - 2.0 * s, 0.0)
        base = dq[:, None] + dq[None, :] + U * (2.0 + dq[:, None] + dq[None, :]) + 2.0 * ds
        darg = 2.0 * (base + U * (d2 + base))
        dk = kk * (np.expm1(darg) + 2 * U * np.exp(darg))
        dks = np.triu(dk, 1).sum()
        dZ = nZ * U * (Z + dks) + dks
        relZ = dZ / Z
        assert relZ < 0.5, relZ
        dunif = -np.log1p(-relZ) + 2 * U + 2 * U * abs(unif) + 1e-37
        coef = 2.0 * gamma / Z
        dcoef = coef * (relZ / (1.0 - relZ) + 3 * U)
        dW = coef * dk + dcoef * (kk + dk) + U * (coef + dcoef) * (kk + dk)
        Wf = Wm + dW
        sf = np.abs(s) + ds
        G_abs = Wf @ h
        dg = (n_chain + 1) * U * G_abs + dW @ h + Wf @ dh
        t_abs = (Wf * sf).sum(1)
        dt = (n_chain + 1) * U * t_abs + (dW * sf).sum(1) + (Wf * ds).sum(1)
        off = inv[:, None] * (dg + dt[:, None] * h + t_abs[:, None] * dh + (3 * U + rho_o)[:, None] * (G_abs + t_abs[:, None] * h))
        return dict(dunif=dunif, relZ=relZ, dZ=dZ, off=off, dq=dq)
    sx = side(x, hx, dhx, r["k_x"].numpy(), r["W_x"].numpy(), float(r["Z_x"]), float(r["unif_x"]), inv_u, rho_u)
    sy = side(y, hy, dhy, r["k_y"].numpy(), r["W_y"].numpy(), float(r["Z_y"]), float(r["unif_y"]), inv_p, rho_p)
    cst = float(r["cst"])
    dcst = 0.5 * gamma * (sx["dunif"] + sy["dunif"]) + 3 * U * abs(cst)

    # ---- the alignment term and its gradient
    dqx = (CPT + 7) * U * (hx * hx).sum(1) + 2 * (hx * dhx).sum(1)
    dqy = (CPT + 7) * U * (hy * hy).sum(1) + 2 * (hy * dhy).sum(1)
    dd = np.abs(x - y)
    ddd = dhx + dhy + U * (dd + dhx + dhy)
    al = r["al"].numpy()
    dal = (CPT + 7) * U * ((dd + ddd) ** 2).sum(1) + (2 * dd * ddd + ddd ** 2).sum(1)
    sxy = (x * y).sum(1)
    dsxy = (CPT + 7) * U * (hx * hy).sum(1) + (dhx * hy + hx * dhy).sum(1)
    tx = np.abs(1.0 - sxy)
    dtx = dqx + dsxy + U * (tx + dqx + dsxy)
    dty = dqy + dsxy + U * (tx + dqy + dsxy)
    w2 = 2.0 / B
    d_ga_u = inv_u[:, None] * w2 * (ddd + dtx[:, None] * hx + tx[:, None] * dhx + (5 * U + rho_u)[:, None] * (dd + ddd + (tx + dtx)[:, None] * hx))
    d_ga_p = inv_p[:, None] * w2 * (ddd + dty[:, None] * hy + tx[:, None] * dhy + (5 * U + rho_p)[:, None] * (dd + ddd + (tx + dty)[:, None] * hy))
    out = {"rho": float(max(rho_u.max(), rho_p.max())), "relZ": (sx["relZ"], sy["relZ"]), "dZ": (sx["dZ"], sy["dZ"])}
    out["term"] = dal + dcst + U * (al + abs(cst) + dal + dcst) + 1e-37
    out["void_term"] = dcst + 1e-37

    # ---- reg term (raw rows)
    if ego:
        e0 = np.abs(E0)
        regterm = (e0[ui] ** 2).sum(1) + (e0[pi] ** 2).sum(1)
        d_regx = 0.0
    else:
        regterm = (au * au).sum(1) + (ap * ap).sum(1)
        d_regx = 2.0 * ((au * du).sum(1) + (ap * dp).sum(1))
    out["regterm"] = (4 * CPT + 12) * U * regterm + d_regx + 1e-37
    cB = c_loss(B) * U
    n_void = B - nb
    b_au = (out["term"].sum() + n_void * out["void_term"]) / B + cB * (np.abs(al + cst).sum() + n_void * abs(cst)) / B
    b_reg = 0.5 * (out["regterm"].sum() / B + cB * regterm.sum() / B)
    lo = [float(v) for v in r["loss_out"]]
    out["loss"] = (b_au + SC.DECAY * b_reg + 4 * U * (abs(lo[1]) + SC.DECAY * abs(lo[2])), b_au, b_reg)

    # ---- gradient rows
    lam = 0.0 if ego else SC.DECAY / B
    fx = (NP + 2) * 2.0 ** -51
    d_gu = sx["off"] + d_ga_u + 6 * U * lam * au + lam * du + fx
    d_gp = sy["off"] + d_ga_p + 6 * U * lam * ap + lam * dp + fx
    dG = np.zeros_like(T)
    np.add.at(dG, ui, d_gu); np.add.at(dG, pi, d_gp)
    div = 1.0 if w is not None else float(K + 1)
    Gref = r["G"].numpy()
    Gs = np.abs(Gref) / div
    dGs = dG / div + 2 * U * Gs
    # ---- backward chain (tests/test_gpu_softmax.py)
    cw = [abs(v_) * div for v_ in wk]
    v = cw[K] * (Gref / div)
    h, dh = np.abs(v), cw[K] * dGs + (U * cw[K] * Gs if w is not None else 0.0)
    D = dh
    for i in range(K):
        k = K - i
        Ah = ab @ h
        D = cw[k - 1] * dGs + ab @ dh + spmm_sum_bound(ab.indptr, ab.data, ab.indices, h + dh, extra_terms=extra) + 2 * U * (cw[k - 1] * Gs + Ah)
        v = (wk[k - 1] * div) * (Gref / div) + bwd @ v
        if i < K - 1 and mode == "bf16":
            D = SC.stored_bound(v, D, "bf16")
        h, dh = np.abs(v), D
    if ego:
        D = D + 4 * U * (SC.DECAY / B) * r["cnt"].numpy()[:, None] * np.abs(E0) + 2 * U * np.abs(r["g_final"].numpy())
    out["g_final"] = D
    return out

