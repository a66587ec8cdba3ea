"""NumPy models of the two QC kernels of csrc/ldpc5g.hip (same tables, same arithmetic,
same order).  They run on the CPU and are compared with the oracle in the ``not gpu``
suite, so that the ALGORITHMS (closed-form RU encoder on rotations; compressed check-node
state of the on-chip min-sum decoder) are validated even where no GPU is available.
They are test code: nothing in the product imports them.
"""
import numpy as np

F = np.float32


def _tables(enc):
    z = enc.z
    rows = enc._bg_rows.astype(int)
    cols = enc._bg_cols.astype(int)
    sh = enc._bg_shifts.astype(int) % z
    mb, nb = (46, 68) if enc._bg == "bg1" else (42, 52)
    by_row = [[] for _ in range(mb)]
    for r, c, s in zip(rows, cols, sh):
        by_row[r].append((c, s))
    for r in range(mb):
        by_row[r].sort()
    return z, mb, nb, by_row


def encode_qc_model(enc, u):
    """Model of ldpc5g_encode_kernel: u [B,k] 0/1 -> c [B,n]."""
    z, mb, nb, by_row = _tables(enc)
    k_b = enc._k_b
    B = u.shape[0]
    cw = np.zeros((B, nb * z), np.uint8)
    cw[:, :enc.k] = u.astype(np.uint8) & 1
    zz = np.arange(z)
    blk = lambda c: cw[:, c * z:(c + 1) * z]
    rot = lambda x, s: x[:, (zz + s) % z]                       # (P_s x)[z] = x[(z+s) mod Z]
    lam = []
    for r in range(4):
        acc = np.zeros((B, z), np.uint8)
        for c, s in by_row[r]:
            if c < k_b:
                acc ^= rot(blk(c), s)
        lam.append(acc)
    find = lambda r, c: [s for cc, s in by_row[r] if cc == c][0]
    s_a = find(0, k_b)
    s_b = find(1 if enc._bg == "bg1" else 2, k_b)
    p0 = rot(lam[0] ^ lam[1] ^ lam[2] ^ lam[3], -s_b)
    ap0 = rot(p0, s_a)
    p1 = lam[0] ^ ap0
    p3 = lam[3] ^ ap0
    p2 = (lam[2] ^ p3) if enc._bg == "bg1" else (lam[1] ^ p1)
    for j, p in enumerate((p0, p1, p2, p3)):
        cw[:, (k_b + j) * z:(k_b + j + 1) * z] = p
    for r in range(4, mb):
        acc = np.zeros((B, z), np.uint8)
        for c, s in by_row[r]:
            if c < k_b + 4:
                acc ^= rot(blk(c), s)
        cw[:, (k_b + r) * z:(k_b + r + 1) * z] = acc
    # rate matching (short_to_full(out_to_short(o)))
    n, k, k_ldpc = enc.n, enc.k, enc.k_ldpc
    o = np.arange(n)
    m = enc.num_bits_per_symbol
    t = o if m is None else (o % m) * (n // m) + o // m
    uu = t + 2 * z
    full = np.where(uu < k, uu, uu + (k_ldpc - k))
    return cw[:, full].astype(np.float32)


def decode_onchip_model(dec, llr, num_iter, offset=0.0):
    """Model of ldpc5g_decode_kernel (one codeword at a time, vectorised over lifted copies).

    dec: sionna_amd LDPC5GDecoder (host object, gives pruning); llr [B,n] logits.
    Returns x_hat internal LLRs clipped [B, N_vn] (callers map to outputs).
    """
    enc = dec.encoder
    z, mb, nb, by_row = _tables(enc)
    n_vn, n_cn = dec.num_vns, dec.num_cns
    llr_max = F(dec.llr_max)
    by_col = [[] for _ in range(nb)]
    for r in range(mb):
        for pos, (c, s) in enumerate(by_row[r]):
            by_col[c].append((r, s, pos))
    # rate recovery (recover_llr)
    B = llr.shape[0]
    k, n, k_ldpc = enc.k, enc.n, enc.k_ldpc
    v = np.arange(n_vn)
    u = np.where(v < k, v, v - (k_ldpc - k))
    t = u - 2 * z
    valid = (t >= 0) & (t < n) & ~((v >= k) & (v < k_ldpc))
    m = enc.num_bits_per_symbol
    tt = np.clip(t, 0, n - 1)
    o = tt if m is None else (tt // (n // m)) + (tt % (n // m)) * m
    rec = np.where(valid[None, :], llr[:, o], F(0))
    rec[:, (v >= k) & (v < k_ldpc)] = -llr_max
    out = np.zeros((B, n_vn), F)
    zz = np.arange(z)
    for b in range(B):
        l = (F(-1) * np.clip(rec[b], -llr_max, llr_max)).astype(F)
        xt = l.copy()
        m1 = np.zeros(n_cn, F); m2 = np.zeros(n_cn, F)
        idxs = np.zeros(n_cn, np.int64); sgn = np.zeros(n_cn, np.int64)
        for _ in range(num_iter):
            for r in range(mb):
                cn = r * z + zz
                act = cn < n_cn
                if not act.any():
                    continue
                cna = cn[act]; za = zz[act]
                d = len(by_row[r])
                min1 = np.full(len(cna), np.inf, F); min2 = np.full(len(cna), np.inf, F)
                idx = np.zeros(len(cna), np.int64); cnt = np.zeros(len(cna), np.int64)
                neg = np.zeros(len(cna), np.int64)
                for i, (c, s) in enumerate(by_row[r]):
                    c2v = np.where(idxs[cna] == i, m2[cna], m1[cna])
                    c2v = np.where((sgn[cna] >> i) & 1, -c2v, c2v)
                    v2c = np.clip(F(-1) * c2v + xt[c * z + (za + s) % z], -llr_max, llr_max).astype(F)
                    neg |= (v2c < 0).astype(np.int64) << i
                    a = np.abs(v2c)
                    lt = a < min1
                    eq = (a == min1) & ~lt
                    lt2 = (a < min2) & ~lt & ~eq
                    min2 = np.where(lt, min1, np.where(lt2, a, min2))
                    idx = np.where(lt, i, idx)
                    cnt = np.where(lt, 1, np.where(eq, cnt + 1, cnt))
                    min1 = np.where(lt, a, min1)
                with np.errstate(invalid="ignore"):
                    min_e = np.where(cnt == 1, (min2 - min1) + min1, min1).astype(F)
                a1 = np.minimum(np.maximum(min1 - F(offset), F(0)), llr_max)
                a2 = np.minimum(np.maximum(min_e - F(offset), F(0)), llr_max)
                par = np.array([bin(x).count("1") & 1 for x in neg])
                allm = (1 << d) - 1
                s_new = np.where(par == 1, ~neg & allm, neg)
                m1[cna], m2[cna], idxs[cna], sgn[cna] = a1, a2, idx, s_new
            new_xt = xt.copy()
            for c in range(nb):
                vn = c * z + zz
                act = vn < n_vn
                if not act.any():
                    continue
                vna = vn[act]; za = zz[act]
                x = np.zeros(len(vna), F)
                for (r, s, pos) in by_col[c]:
                    cn = r * z + (za - s) % z
                    ok = cn < n_cn
                    cnc = np.where(ok, cn, 0)
                    c2v = np.where(idxs[cnc] == pos, m2[cnc], m1[cnc])
                    c2v = np.where((sgn[cnc] >> pos) & 1, -c2v, c2v)
                    x = np.where(ok, x + c2v, x).astype(F)
                new_xt[vna] = x + l[vna]
            xt = new_xt
        out[b] = np.clip(xt, -llr_max, llr_max)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cir_to_ofdm_channel (csrc/ofdm.hip): integer models of the host dispatcher and of the pass kernel's row ownership, and a
# float32 restatement of the kernels' summation orders.  Held to tests/channel_f32.py in tests/test_kernel_models.py.
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _c2o_block(rows, nf):
    """the block size search shared by samd_cir_to_ofdm_c64 and samd_ofdm_channel_fused_c64 -> (nt, rpt) or (0, 0)"""
    best_nt, best_rpt, best_u = 0, 0, 0.0
    if nf <= 512:
        for nt in range(256, 513, 64):
            if nf > nt:
                continue
            gq = nt // nf
            rpt = (rows + gq - 1) // gq
            u = (gq * nf) / nt
            if rpt <= 40 and u > best_u + 1e-9:
                best_u, best_nt, best_rpt = u, nt, rpt
    return best_nt, best_rpt


def c2o_dispatch(RA, TA, P, T, nf, num_tx=1, pass_width=4, two_pass=False):
    """Which kernel samd_cir_to_ofdm_c64 launches for a link of RA x TA antennas, P paths, T time steps and nf subcarriers, and
    whether samd_ofdm_channel_fused_c64 accepts the shape (one transmitter) - the host code restated in integers.
    ``pass_width`` / ``two_pass``: the development switches SAMD_C2O_PASS / SAMD_C2O_TWO_PASS."""
    rows = RA * TA * T
    nt, rpt = _c2o_block(rows, nf)
    mp = 8 if P <= 8 else 16 if P <= 16 else 24 if P <= 24 else 32 if P <= 32 else 0
    small = P * T * RA * TA < 8192
    out = dict(fused=False)
    if nt and mp:
        G, rpt_pad = nt // nf, (rpt + 7) // 8 * 8
        lds_p = (mp * nf + rpt_pad * G * mp) * 8 + 64
        lds_f = max(lds_p, TA * T * nf * 8 + 64)
        lds_r = (mp * nf + RA * TA * mp * T) * 8 + 512 * 4
        out["fused"] = bool(num_tx == 1 and lds_r <= 64 * 1024 and lds_f <= 64 * 1024 and small and rpt_pad % TA == 0
                            and (rpt_pad // TA) * G >= RA * T)
        if lds_r <= 64 * 1024 and not two_pass:
            is_pass = pass_width in (8, 4, 2) and lds_p <= 64 * 1024 and small
            out.update(family="pass" if is_pass else "reg", nt=nt, G=G, RPT=rpt_pad, MAXP=mp,
                       grouped=bool(is_pass and rpt_pad % TA == 0), taps_lds=True, spare=nt - G * nf)
            return out
    tab_b = P * nf * 8 + 256 * 4
    taps_b = RA * TA * P * T * 8
    assert tab_b <= 160 * 1024, "phase table (num_paths x num_freqs) exceeds the LDS"
    G = 256 // nf if nf <= 256 else 1
    out.update(family="two_pass", nt=256, G=G, RPT=None, MAXP=mp if mp else 64 if P <= 64 else 0, grouped=False,
               taps_lds=tab_b + taps_b <= 160 * 1024, spare=256 - G * nf if nf <= 256 else 0)
    return out


def c2o_magic(d):
    """the pass kernel's ``magic``: 0xFFFFFFFF / d + 1 in 32 bits (d = 1 wraps to 0 and is never multiplied)"""
    return ((M32 // d) + 1) & M32 if d > 1 else 0


def c2o_divu(n, d, m):
    """``divu``: __umulhi(n, m) for d > 1, else n; n a uint64 array of 32-bit values"""
    n = np.asarray(n, np.uint64)
    assert np.all(n <= M32)
    return (n * np.uint64(m)) >> np.uint64(32) if d > 1 else n


def c2o_stage_rows(RA, TA, P, T, G, RPT, pp):
    """Staging of the pass kernel for the taps of path ``pp``: the source index i of every (ra, ta, t), decomposed with the
    kernel's multiply-high divisions in 32-bit arithmetic -> (lk, t, row) arrays in source order, row the tap-table row."""
    grouped = RPT % TA == 0
    pt, lpt = P * T, TA * P * T
    m_pt, m_t, m_ta, m_g = c2o_magic(pt), c2o_magic(T), c2o_magic(TA), c2o_magic(G)
    lk0 = np.repeat(np.arange(RA * TA, dtype=np.uint64), T)
    t0 = np.tile(np.arange(T, dtype=np.uint64), RA * TA)
    i = lk0 * np.uint64(pt) + np.uint64(pp * T) + t0
    assert int(i.max()) < RA * lpt
    w = np.uint64(M32)
    lk = c2o_divu(i, pt, m_pt)
    q = (i - lk * np.uint64(pt)) & w
    p_ = c2o_divu(q, T, m_t)
    t = (q - p_ * np.uint64(T)) & w
    assert np.array_equal(p_, np.full_like(p_, pp))
    row = (lk * np.uint64(T) + t) & w
    if grouped:
        ra = c2o_divu(lk, TA, m_ta)
        ta = (lk - ra * np.uint64(TA)) & w
        u = (ra * np.uint64(T) + t) & w
        j = c2o_divu(u, G, m_g)
        row = ((u - j * np.uint64(G)) + (j * np.uint64(TA) + ta) * np.uint64(G)) & w
    return lk.astype(np.int64), t.astype(np.int64), row.astype(np.int64)


def c2o_row_walk(RA, TA, T, G, RPT, grouped):
    """``RowWalk`` for every group g at once: -> ra, ta, t int arrays [G, RPT], what ``init`` and RPT - 1 ``step`` report for
    result register r of group g (a result is stored where ra < RA)"""
    m = c2o_magic(T)
    g = np.arange(G, dtype=np.int64)
    o_ra, o_ta, o_t = (np.zeros((G, RPT), np.int64) for _ in range(3))

    def div_t(u):
        return c2o_divu(u.astype(np.uint64), T, m).astype(np.int64)
    if grouped:
        u, ta = g.copy(), np.zeros(G, np.int64)
        ra = div_t(u)
        t = u - ra * T
    else:
        u = None
        t, ta, ra = g % T, (g // T) % TA, (g // T) // TA
    for r in range(RPT):
        o_ra[:, r], o_ta[:, r], o_t[:, r] = ra, ta, t
        if grouped:
            ta = ta + 1
            if ta[0] == TA:                                          # wave-uniform: the same for every group
                ta = np.zeros(G, np.int64)
                u = u + G
                ra = div_t(u)
                t = u - ra * T
        else:
            t = t + G
            while True:
                over = t >= T
                if not over.any():
                    break
                t = np.where(over, t - T, t)
                ta = np.where(over, ta + 1, ta)
                carry = over & (ta == TA)
                ta = np.where(carry, 0, ta)
                ra = np.where(carry, ra + 1, ra)
    return o_ra, o_ta, o_t


def c2o_owned_rows(RA, TA, T, d):
    """int [G, rpt]: the row (ra TA + ta) T + t whose result sits in register r of group g, -1 for none, for the dispatch ``d``
    of c2o_dispatch: the order in which a thread adds up its share of the link's energy"""
    G, rows = d["G"], RA * TA * T
    if d["family"] == "pass":
        ra, ta, t = c2o_row_walk(RA, TA, T, G, d["RPT"], d["grouped"])
        return np.where(ra < RA, (ra * TA + ta) * T + t, -1)
    rpt = -(-rows // G)
    r = np.arange(G)[:, None] + np.arange(rpt)[None, :] * G
    return np.where(r < rows, r, -1)


def _fma(x, y, z):
    """float32 fused multiply-add through float64: the product of two float32 is exact there, the sum is rounded to float64 and
    then to float32 - a double rounding that differs from the fused result in rare ties (accepted: the models are held to a
    bound, not to bits)"""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


C2O_MUTATIONS = ("drop_weakest", "flip_sin", "tau_next_tx", "next_row_taps", "inv_neighbour", "f_off_by_one")


def c2o_model_f32(freqs, a, tau, normalize, d, chain=None, mutation=None, spacing=15e3):
    """Float32 restatement of cir_to_ofdm_channel for the dispatch ``d`` (c2o_dispatch): phases from host sin / cos of the
    float32 argument, rounded to float32; the sum over the paths as the kernel family chains it; the energy reduced in the
    family's order.  chain: "one" (two-pass kernel: one accumulator, 2 fused multiply-adds per path and component), "uv"
    (register-staged kernel: real-tap and imaginary-tap accumulators joined at the end), "pass" (pass kernel: one accumulator
    over zero-padded passes of 4).  ``mutation``: one of C2O_MUTATIONS - a seeded fault that the bound has to catch."""
    f32 = np.float32
    freqs, a, tau = np.asarray(freqs, f32), np.asarray(a, np.complex64), np.asarray(tau, f32)
    b, rx, ra_n, tx, ta_n, p_n, t_n = a.shape
    nf = freqs.size
    chain = chain or {"two_pass": "one", "reg": "uv", "pass": "pass"}[d["family"]]
    if mutation == "drop_weakest":
        a = a.copy()
        a[:, :, :, :, :, int(np.argmin(np.sum(np.abs(a) ** 2, axis=(0, 1, 2, 3, 4, 6))))] = 0
    if mutation == "tau_next_tx":
        tau = np.roll(tau, -1, axis=2)
    if mutation == "next_row_taps":                                  # the row behind the last real row is a padded zero row
        a = a.copy()
        a[:, :, -1, :, -1, :, -1] = 0
    if mutation == "f_off_by_one":
        freqs = (freqs + f32(spacing)).astype(f32)
    wf = (f32(-2.0) * f32(3.14159265358979323846)) * freqs                       # float32 [F]
    arg = (wf[None, None, None, None, :] * tau[..., None]).astype(f32)           # [b, rx, tx, p, F]
    assert arg.dtype == f32
    cs = np.cos(arg.astype(np.float64)).astype(f32)
    sn = np.sin(arg.astype(np.float64)).astype(f32)
    if mutation == "flip_sin":
        sn[:, :, :, p_n // 2] = -sn[:, :, :, p_n // 2]
    ax = np.ascontiguousarray(a.real)[..., None]                                 # [b, rx, ra, tx, ta, p, t, 1]
    ay = np.ascontiguousarray(a.imag)[..., None]

    def ph(v, p):                                                                # -> [b, rx, 1, tx, 1, 1, F]
        return v[:, :, None, :, None, p, None, :]
    shape = (b, rx, ra_n, tx, ta_n, t_n, nf)
    zero = np.zeros(shape, f32)
    if chain == "uv":
        ux, uy, vx, vy = zero, zero, zero, zero
        for p in range(p_n):                                         # (a padded path adds 0 * 0 to an accumulator: exact)
            c_, s_ = ph(cs, p), ph(sn, p)
            ux, uy = _fma(ax[:, :, :, :, :, p], c_, ux), _fma(ax[:, :, :, :, :, p], s_, uy)
            vx, vy = _fma(ay[:, :, :, :, :, p], s_, vx), _fma(ay[:, :, :, :, :, p], c_, vy)
        hx, hy = ux - vx, uy + vy
    else:
        hx, hy = zero, zero
        maxp = max(d["MAXP"], -(-p_n // 4) * 4) if chain == "pass" else p_n
        pw = 4 if chain == "pass" else 1
        zc = np.zeros((b, rx, 1, tx, 1, 1, nf), f32)
        za = np.zeros(ax[:, :, :, :, :, 0].shape, f32)
        for p0 in range(0, maxp, pw):                                # pass by pass, the accumulator carried across
            for p in range(p0, p0 + pw):
                real = p < p_n
                c_, s_ = (ph(cs, p), ph(sn, p)) if real else (zc, zc)
                axp, ayp = (ax[:, :, :, :, :, p], ay[:, :, :, :, :, p]) if real else (za, za)
                hx, hy = _fma(axp, c_, hx), _fma(axp, s_, hy)
                hx, hy = _fma(ayp, -s_, hx), _fma(ayp, c_, hy)
    assert hx.dtype == f32 and hy.dtype == f32
    h = np.empty(shape, np.complex64)
    h.real, h.imag = hx, hy
    if not normalize:
        return h
    # energy: per thread (g, f) serially over its rows, then across the block
    own = c2o_owned_rows(ra_n, ta_n, t_n, d)                                     # [G, rpt]
    G, nt = d["G"], d["nt"]
    e_row = (hx * hx + hy * hy).astype(f32)                                      # fl(fl(x^2) + fl(y^2))
    e_row = np.moveaxis(e_row, 3, 2).reshape(b, rx, tx, ra_n * ta_n * t_n, nf)   # [b, rx, tx, row, F]
    lanes = np.zeros((b, rx, tx, nt), f32)
    if nf <= nt:
        part = np.zeros((b, rx, tx, G, nf), f32)
        for r in range(own.shape[1]):
            idx = own[:, r]
            term = np.where((idx >= 0)[:, None], e_row[:, :, :, np.maximum(idx, 0), :], f32(0))
            part = part + term
        lanes[..., :G * nf] = part.reshape(b, rx, tx, G * nf)
    else:                                                            # two-pass kernel, F > blockDim: f = f0 + tid, all rows
        for f0 in range(0, nf, nt):
            w = min(nt, nf - f0)
            for r in range(e_row.shape[3]):
                lanes[..., :w] = lanes[..., :w] + e_row[:, :, :, r, f0:f0 + w]
    assert lanes.dtype == f32
    if d["family"] == "pass":                                        # xor butterfly in a wave, then the waves in order
        x = lanes.reshape(b, rx, tx, nt // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            x = x + x[..., lane ^ o]
        e = np.zeros((b, rx, tx), f32)
        for wv in range(nt // 64):
            e = e + x[..., wv, 0]
    else:                                                            # LDS tree over the next power of two
        x = lanes.copy()
        o = 1
        while o < nt:
            o <<= 1
        if d["family"] == "two_pass":
            o = 256
        o >>= 1
        while o > 0:
            hi = min(o, nt - o)
            if hi > 0:
                x[..., :hi] = x[..., :hi] + x[..., o:o + hi]
            o >>= 1
        e = x[..., 0]
    c = np.sqrt((e / f32(ra_n * ta_n * t_n * nf)).astype(f32)).astype(f32)
    with np.errstate(divide="ignore"):
        inv = np.where(c > 0, f32(1) / np.where(c > 0, c, f32(1)), f32(0)).astype(f32)
    if mutation == "inv_neighbour":
        inv = np.roll(inv.reshape(-1), 1).reshape(inv.shape)
    inv = inv[:, :, None, :, None, None, None]
    h.real, h.imag = hx * inv, hy * inv
    return h
