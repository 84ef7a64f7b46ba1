"""Lane-level emulation of the index algebra of the bf16 attention kernels (csrc/vt_attention.hip), on the CPU in numpy.

    python tools/attn_lane_emulation.py

It restates, lane by lane, which element of every `mfma_f32_16x16x32_bf16` operand and result a lane holds (A[row = lane & 15]
[k = 8 (lane >> 4) + j], B[k][col = lane & 15], D[row = 4 (lane >> 4) + r][col = lane & 15]), which rows the transposing LDS read
`ds_read_b64_tr_b16` hands a lane (rows R..R+3 of column d0 + (lane & 15), R per 16-lane group), and how the forward, the dK / dV
pass and the dQ pass chain them: scores taken transposed, the accumulator tile packed as the next product's B operand in the
permuted row order 32 s + 16 (j >> 2) + 4 g + (j & 3), tiles zero padded beyond L.  Values are float64 and nothing is rounded:
the printed differences against the dense computation must be at rounding level (1e-15), which shows that the index maps are
consistent with each other and with the tails (L = 70, head_dim 32: two key tiles, the second with 6 rows).  It says nothing
about rounding, alignment or speed -- tests/test_attention_gpu.py does that on the GPU.
"""
import numpy as np
rng = np.random.default_rng(0)
D, L, P = 32, 70, 40
scale = D ** -0.5
Q, K, V, G = (rng.standard_normal((L, D)) for _ in range(4))

def mfma(A, B, Cacc):
    # A[lane] (8,), B[lane] (8,), C[lane] (4,): lane=(g,u); A[row=u][k=8g+j], B[k=8g+j][col=u], D[row=4g+r][col=u]
    Am = np.zeros((16, 32)); Bm = np.zeros((32, 16))
    for g in range(4):
        for u in range(16):
            Am[u, 8*g:8*g+8] = A[g*16+u]; Bm[8*g:8*g+8, u] = B[g*16+u]
    Dm = Am @ Bm
    out = Cacc.copy()
    for g in range(4):
        for u in range(16):
            out[g*16+u] += Dm[4*g:4*g+4, u]
    return out

def stage(X, row0):
    T = np.zeros((64, P))
    for r in range(64):
        if row0 + r < L: T[r, :D] = X[row0 + r]
    return T
def frag_lds(T, rowbase, kk):  # per lane: row = rowbase+u
    return np.array([T[rowbase + (l & 15), 32*kk + 8*(l >> 4): 32*kk + 8*(l >> 4) + 8] for l in range(64)])
def frag_glob(X, row0, kk):
    out = np.zeros((64, 8))
    for l in range(64):
        r = row0 + (l & 15)
        if r < L: out[l] = X[r, 32*kk + 8*(l >> 4): 32*kk + 8*(l >> 4) + 8]
    return out
def tr(T, R0_of_lane, d0):
    # lane (g,u) gets rows R0..R0+3 (R0 per 16-lane group) of column d0+u
    return np.array([[T[R0_of_lane(l >> 4) + e, d0 + (l & 15)] for e in range(4)] for l in range(64)])
def frag_tr(T, s, d0):
    lo = tr(T, lambda g: 32*s + 4*g, d0); hi = tr(T, lambda g: 32*s + 4*g + 16, d0)
    return np.concatenate([lo, hi], 1)
def pack8(a, b): return np.concatenate([a, b], 1)

S = scale * Q @ K.T; Pm = np.exp(S - S.max(1, keepdims=True)); Pm /= Pm.sum(1, keepdims=True)
O_ref = Pm @ V; lse_ref = np.log(np.exp(S).sum(1))
dP = G @ V.T; delta = (G * O_ref).sum(1); dS = Pm * (dP - delta[:, None])
dQ_ref, dK_ref, dV_ref = scale * dS @ K, scale * dS.T @ Q, Pm.T @ G

# forward, wave by wave
O = np.zeros((L, D)); lse = np.zeros(L)
for qt in range(0, L, 64):
  for wave in range(4):
    q0 = qt + wave*16
    qf = [frag_glob(Q, q0, kk) for kk in range(D//32)]
    o = [np.zeros((64, 4)) for _ in range(D//16)]; m = np.full(64, -np.inf); l_ = np.zeros(64)
    for k0 in range(0, L, 64):
        Ks, Vs = stage(K, k0), stage(V, k0)
        s = []
        for t in range(4):
            acc = np.zeros((64, 4))
            for kk in range(D//32): acc = mfma(frag_lds(Ks, 16*t, kk), qf[kk], acc)
            for ln in range(64):
                for r in range(4):
                    acc[ln, r] = acc[ln, r]*scale if k0 + 16*t + 4*(ln >> 4) + r < L else -np.inf
            s.append(acc)
        mx = np.max(np.concatenate(s, 1), 1)
        mx = np.array([max(mx[(ln & 15) + 16*g] for g in range(4)) for ln in range(64)])
        mn = np.maximum(m, mx); alpha = np.exp(m - mn)
        s = [np.exp(a - mn[:, None]) for a in s]
        rs = np.concatenate(s, 1).sum(1); rs = np.array([sum(rs[(ln & 15) + 16*g] for g in range(4)) for ln in range(64)])
        l_ = l_*alpha + rs; m = mn
        o = [a*alpha[:, None] for a in o]
        for ks in range(2):
            pf = pack8(s[2*ks], s[2*ks+1])
            for i in range(D//16): o[i] = mfma(frag_tr(Vs, ks, 16*i), pf, o[i])
    for ln in range(64):
        g, u = ln >> 4, ln & 15
        if q0 + u < L:
            for i in range(D//16): O[q0+u, 16*i + 4*g: 16*i + 4*g + 4] = o[i][ln] / l_[ln]
            lse[q0+u] = m[ln] + np.log(l_[ln])
print("fwd", np.abs(O - O_ref).max(), np.abs(lse - lse_ref).max())

dK = np.zeros((L, D)); dV = np.zeros((L, D)); dQ = np.zeros((L, D))
for kt in range(0, L, 64):
  for wave in range(4):
    key0 = kt + wave*16
    kf = [frag_glob(K, key0, kk) for kk in range(D//32)]; vf = [frag_glob(V, key0, kk) for kk in range(D//32)]
    dk = [np.zeros((64, 4)) for _ in range(D//16)]; dv = [np.zeros((64, 4)) for _ in range(D//16)]
    for q0 in range(0, L, 64):
        Qs, Gs = stage(Q, q0), stage(G, q0)
        s, dp = [], []
        for t in range(4):
            a = np.zeros((64, 4)); b = np.zeros((64, 4))
            for kk in range(D//32):
                a = mfma(frag_lds(Qs, 16*t, kk), kf[kk], a); b = mfma(frag_lds(Gs, 16*t, kk), vf[kk], b)
            for ln in range(64):
                g, u = ln >> 4, ln & 15
                for r in range(4):
                    qi = q0 + 16*t + 4*g + r
                    ok = key0 + u < L and qi < L
                    pr = np.exp(a[ln, r]*scale - lse_ref[qi]) if ok else 0.0
                    a[ln, r] = pr; b[ln, r] = pr*(b[ln, r] - (delta[qi] if qi < L else 0))
            s.append(a); dp.append(b)
        for ks in range(2):
            pf, df = pack8(s[2*ks], s[2*ks+1]), pack8(dp[2*ks], dp[2*ks+1])
            for i in range(D//16):
                dv[i] = mfma(frag_tr(Gs, ks, 16*i), pf, dv[i]); dk[i] = mfma(frag_tr(Qs, ks, 16*i), df, dk[i])
    for ln in range(64):
        g, u = ln >> 4, ln & 15
        if key0 + u < L:
            for i in range(D//16):
                dK[key0+u, 16*i+4*g:16*i+4*g+4] = dk[i][ln]*scale; dV[key0+u, 16*i+4*g:16*i+4*g+4] = dv[i][ln]
print("dK", np.abs(dK - dK_ref).max(), "dV", np.abs(dV - dV_ref).max())
for qt in range(0, L, 64):
  for wave in range(4):
    q0 = qt + wave*16
    qf = [frag_glob(Q, q0, kk) for kk in range(D//32)]; gf = [frag_glob(G, q0, kk) for kk in range(D//32)]
    dq = [np.zeros((64, 4)) for _ in range(D//16)]
    for k0 in range(0, L, 64):
        Ks, Vs = stage(K, k0), stage(V, k0)
        ds = []
        for t in range(4):
            a = np.zeros((64, 4)); b = np.zeros((64, 4))
            for kk in range(D//32):
                a = mfma(frag_lds(Ks, 16*t, kk), qf[kk], a); b = mfma(frag_lds(Vs, 16*t, kk), gf[kk], b)
            for ln in range(64):
                g, u = ln >> 4, ln & 15
                for r in range(4):
                    ok = q0 + u < L and k0 + 16*t + 4*g + r < L
                    pr = np.exp(a[ln, r]*scale - lse_ref[q0+u]) if ok else 0.0
                    b[ln, r] = pr*(b[ln, r] - (delta[q0+u] if q0+u < L else 0))
            ds.append(b)
        for ks in range(2):
            df = pack8(ds[2*ks], ds[2*ks+1])
            for i in range(D//16): dq[i] = mfma(frag_tr(Ks, ks, 16*i), df, dq[i])
    for ln in range(64):
        g, u = ln >> 4, ln & 15
        if q0 + u < L:
            for i in range(D//16): dQ[q0+u, 16*i+4*g:16*i+4*g+4] = dq[i][ln]*scale
print("dQ", np.abs(dQ - dQ_ref).max())
assert max(np.abs(O - O_ref).max(), np.abs(lse - lse_ref).max(), np.abs(dK - dK_ref).max(), np.abs(dV - dV_ref).max(),
           np.abs(dQ - dQ_ref).max()) < 1e-12
