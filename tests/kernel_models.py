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


# ---------------------------------------------------------------------------------------------------------------------
# cir_to_time_channel / ApplyTimeChannel (csrc/ofdm_time.hip): float32 restatements of cir_to_time_kernel and
# apply_time_kernel in their summation order, the LDS stages as their index arithmetic on a flat array.  Held to
# tests/time_channel_f32.py in tests/test_time_channel_host.py.  The library is built without contraction: a product and a
# sum are one rounding each, which is what NumPy's float32 operations do.
# ---------------------------------------------------------------------------------------------------------------------
C2T_TILE = 9
C2T_MUTATIONS = ("tail_tile_prev_weight", "stage_stride_minus", "stage_stride_plus", "cnt_short_row", "tau_next_tx", "table_unpadded",
                 "mean_over_l")


def c2t_lds_bytes(P, L):
    """LDS of a cir_to_time_kernel workgroup as samd_cir_to_time_c64 counts it: the sinc table padded to an even count, four wave
    stages of [64][L] float2, and the kernel's static red[256]"""
    return ((P * L + 1) & ~1) * 4 + 4 * 64 * L * 8 + 256 * 4


def c2t_model_f32(bandwidth, a, tau, l_min, l_max, normalize, defer=False, mutation=None):
    """cir_to_time_kernel: one workgroup per (b, rx, tx); the sinc table g[p][l] at the start of the LDS, the per-wave stage
    [64][L] of float2 behind it at the float offset (P L + 1) & ~1; per link and per pass of 64 time steps a wave computes lags in
    tiles of 9 (p ascending), writes them to the stage at lane * L + l and copies min(64, T - t0) * L contiguous values out; a
    thread's energy chain runs over everything it computed, the 256 chains meet in a tree.  -> h complex64, or (h unnormalised,
    scale [b, rx, tx]) with ``defer``.  ``mutation``: one of C2T_MUTATIONS - a seeded fault that the bound has to catch.
    "table_unpadded" puts the stage at P L; an 8-byte LDS access ignores the low three address bits, so for odd P L stage[0]
    lands on the last weight of the table."""
    f32 = np.float32
    a, tau = np.asarray(a, np.complex64), np.asarray(tau, f32)
    b_n, rx_n, ra_n, tx_n, ta_n, p_n, t_n = a.shape
    L = l_max - l_min + 1
    grp = b_n * rx_n * tx_n
    nlk = ra_n * ta_n
    ag = np.ascontiguousarray(a.transpose(0, 1, 3, 2, 4, 5, 6)).reshape(grp, nlk, p_n, t_n)
    ax, ay = np.ascontiguousarray(ag.real), np.ascontiguousarray(ag.imag)
    if mutation == "tau_next_tx":
        tau = np.roll(tau, -1, axis=2)
    tg = tau.reshape(grp, p_n)
    # the table
    lag = (l_min + np.arange(L)).astype(f32)
    x = (lag[None, None, :] - (tg * f32(bandwidth))[:, :, None]).astype(f32)     # [grp, P, L]
    y = (f32(3.14159265358979323846) * x).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(x == 0, f32(1), np.sin(y.astype(np.float64)).astype(f32) / np.where(x == 0, f32(1), y)).astype(f32)
    stride = L + {"stage_stride_minus": -1, "stage_stride_plus": 1}.get(mutation, 0)
    base = p_n * L if mutation == "table_unpadded" else (p_n * L + 1) & ~1
    base &= ~1                                                                   # float2 accesses are 8-byte aligned
    lds = np.zeros((grp, base + 2 * (4 * 64 * L + 64 * (abs(stride - L) + 1))), f32)
    lds[:, :p_n * L] = g.reshape(grp, p_n * L)
    hx = np.zeros((grp, nlk, t_n * L), f32)
    hy = np.zeros((grp, nlk, t_n * L), f32)
    energy = np.zeros((grp, 256), f32)
    lane = np.arange(64)
    for lk in range(nlk):
        for tb in range(0, t_n, 256):
            for wv in range(4):
                t0 = tb + 64 * wv
                if t0 >= t_n:
                    continue
                t = t0 + lane
                live = t < t_n
                tc = np.minimum(t, t_n - 1)
                sb = base + 2 * wv * 64 * L
                for l0 in range(0, L, C2T_TILE):
                    nj = min(C2T_TILE, L - l0)
                    j = np.arange(nj)
                    src = l0 - C2T_TILE if (mutation == "tail_tile_prev_weight" and nj < C2T_TILE and l0 > 0) else l0
                    re = np.zeros((grp, 64, nj), f32)
                    im = np.zeros((grp, 64, nj), f32)
                    for p in range(p_n):
                        w = lds[:, p * L + src:p * L + src + nj][:, None, :]     # read from the LDS: a clobbered weight shows
                        vx = np.where(live, ax[:, lk, p, tc], f32(0))[:, :, None]
                        vy = np.where(live, ay[:, lk, p, tc], f32(0))[:, :, None]
                        re = re + vx * w
                        im = im + vy * w
                    assert re.dtype == f32
                    off = sb + 2 * (lane[:, None] * stride + l0 + j[None, :])    # [64, nj] float offsets of the float2
                    lds[:, off] = re
                    lds[:, off + 1] = im
                    for k in range(nj):                                          # zero for t >= T
                        energy[:, 64 * wv:64 * wv + 64] += re[:, :, k] * re[:, :, k] + im[:, :, k] * im[:, :, k]
                rows = min(64, t_n - t0)
                if mutation == "cnt_short_row" and rows < 64:
                    rows -= 1
                cnt = rows * L
                i = np.arange(cnt)
                hx[:, lk, t0 * L + i] = lds[:, sb + 2 * i]
                hy[:, lk, t0 * L + i] = lds[:, sb + 2 * i + 1]

    def out(vx, vy):
        h = np.empty((grp, nlk, t_n * L), np.complex64)
        h.real, h.imag = vx, vy
        h = h.reshape(b_n, rx_n, tx_n, ra_n, ta_n, t_n, L).transpose(0, 1, 3, 2, 4, 5, 6)
        return np.ascontiguousarray(h)
    if not normalize:
        return (out(hx, hy), None) if defer else out(hx, hy)
    red = energy.copy()
    s = 128
    while s > 0:
        red[:, :s] = red[:, :s] + red[:, s:2 * s]
        s >>= 1
    n = nlk * t_n * (L if mutation == "mean_over_l" else 1)
    c = np.sqrt((red[:, 0] / f32(n)).astype(f32)).astype(f32)
    inv = np.where(c > 0, f32(1) / np.where(c > 0, c, f32(1)), f32(0)).astype(f32)
    if defer:
        return out(hx, hy), inv.reshape(b_n, rx_n, tx_n)
    return out(hx * inv[:, None, None], hy * inv[:, None, None])


APT_MUTATIONS = ("hi_short", "lo_late", "lo_early", "x_shift", "scale_other_tx")


def apt_model_f32(x, h, link_scale=None, mutation=None):
    """apply_time_kernel: one lane per output time step, 256 per block; per link (tx outer, ta inner) the block's 256 x L taps are
    one contiguous piece of h, staged at hs[i] and read back at hs[lane * L + l]; l ascending from lo = max(0, t - (Tn - 1)) to
    hi = min(t, L - 1); one accumulator pair over all links.  x is read through its flat storage, as the kernel's pointer
    arithmetic does.  ``mutation``: one of APT_MUTATIONS."""
    f32 = np.float32
    x, h = np.asarray(x, np.complex64), np.asarray(h, np.complex64)
    b_n, rx_n, ra_n, tx_n, ta_n, tout, L = h.shape
    tn = tout - L + 1
    xf = np.concatenate([x.reshape(-1), np.zeros(2, np.complex64)])              # the flat storage, two zeros behind it
    xfx, xfy = np.ascontiguousarray(xf.real), np.ascontiguousarray(xf.imag)
    hf = h.reshape(b_n, rx_n, ra_n, tx_n, ta_n, tout * L)
    yx = np.zeros((b_n, rx_n, ra_n, tout), f32)
    yy = np.zeros((b_n, rx_n, ra_n, tout), f32)
    bi = np.arange(b_n)[:, None, None, None]
    for t0 in range(0, tout, 256):
        nt = min(256, tout - t0)
        tl = np.arange(nt)
        t = t0 + tl
        lo = np.maximum(t - (tn - 1), 0)
        hi = np.minimum(t, L - 1)
        if mutation == "hi_short":
            hi = hi - 1
        if mutation == "lo_late":
            lo = lo + 1
        if mutation == "lo_early":
            lo = np.maximum(t - tn, 0)
        re = np.zeros((b_n, rx_n, ra_n, nt), f32)
        im = np.zeros((b_n, rx_n, ra_n, nt), f32)
        for tx in range(tx_n):
            sc = None
            if link_scale is not None:
                stx = (tx + 1) % tx_n if mutation == "scale_other_tx" else tx
                sc = np.asarray(link_scale, f32)[:, :, stx][:, :, None, None]
            for ta in range(ta_n):
                hs = hf[:, :, :, tx, ta, t0 * L:t0 * L + nt * L]                 # the stage: cnt = nt * L contiguous values
                for l in range(L):
                    on = (l >= lo) & (l <= hi)
                    hv = hs[..., tl * L + l]
                    hvx, hvy = hv.real, hv.imag
                    if sc is not None:
                        hvx, hvy = hvx * sc, hvy * sc
                    xi = (bi * tx_n * ta_n + tx * ta_n + ta) * tn + np.maximum(t - l + (1 if mutation == "x_shift" else 0), 0)
                    xi = np.minimum(np.broadcast_to(xi, (b_n, 1, 1, nt)), xf.size - 1)   # (lanes outside the window read nothing)
                    xvx, xvy = xfx[xi], xfy[xi]
                    re = np.where(on, re + (hvx * xvx - hvy * xvy), re)
                    im = np.where(on, im + (hvx * xvy + hvy * xvx), im)
        assert re.dtype == f32 and im.dtype == f32
        yx[..., t0:t0 + nt], yy[..., t0:t0 + nt] = re, im
    y = np.empty((b_n, rx_n, ra_n, tout), np.complex64)
    y.real, y.imag = yx, yy
    return y


# ------------------------------------------------------------------ TDL / CDL tap generators (csrc/ofdm.hip, csrc/cdl.hip)
def _uni32(seed, call, n, lo, hi):
    """``uni`` / ``unir<float>``: lo + (hi - lo) * u01(word i % 4 of Philox block i / 4), every operation in float32"""
    from oracle import utils as outil
    w = np.stack(outil.philox_block(seed, call, (n + 3) // 4), axis=1).reshape(-1)[:n]
    lo, hi = F(lo), F(hi)
    return (lo + (hi - lo) * outil._u01(w)).astype(F)


PI_F = F(3.14159265358979323846)


def tdl_cir_model(seed, call, batch, num_time_steps, sampling_frequency, mean_powers, min_doppler, max_doppler, num_rx_ant=1,
                  num_tx_ant=1, num_sinusoids=20, los_power=None, los_aoa=np.pi / 4, fault=None):
    """Model of tdl_cir_kernel in float32, operation for operation: chunks of 16 time steps, the first step of a chunk evaluated
    directly, the others by the packed rotation v <- v cw + (-v.y, v.x) sw; the draws once per thread (N <= 24) or once per chunk.
    ``fault``: a seeded one-line fault (tests/test_tap_channel_host.py).  -> complex64 [B, 1, RA, 1, TA, P, T]"""
    b_, ra, ta, t_, n_ = int(batch), int(num_rx_ant), int(num_tx_ant), int(num_time_steps), int(num_sinusoids)
    mp = np.asarray(mean_powers, F)
    p_ = len(mp)
    fs = F(sampling_frequency)
    pi = F(np.nextafter(PI_F, F(4))) if fault == "pi_ulp" else PI_F
    kchunk, kmaxsin = 16, 24
    doppler = _uni32(seed, call, b_, min_doppler, max_doppler).reshape(b_, 1, 1, 1)
    fn = F(n_)
    theta_all = _uni32(seed, call + 1, b_ * p_ * n_, -pi / fn, pi / fn).reshape(b_, 1, 1, p_, n_)
    phi_all = _uni32(seed, call + 2, b_ * ra * ta * p_ * n_, -pi, pi).reshape(b_, ra, ta, p_, n_)
    phi0 = _uni32(seed, call + 3, b_, -pi, pi).reshape(b_, 1, 1)
    amp = np.sqrt(mp).reshape(1, 1, 1, p_)
    norm = F(1) / np.sqrt(fn)
    cached = n_ <= kmaxsin

    def draw(n):
        theta = theta_all[..., n]
        if fault == "theta_no_p" and not cached:                                   # (b * N + n) instead of ((b * P + p) * N + n)
            flat = theta_all.reshape(-1)
            theta = flat[(np.arange(b_) * n_ + n)].reshape(b_, 1, 1, 1) * np.ones((1, 1, 1, p_), F)
        return np.cos((F(2) * PI_F / fn) * F(n + 1) + theta).astype(F), phi_all[..., n]

    out = np.zeros((b_, ra, ta, p_, t_), np.complex64)
    los = los_power is not None
    p_los = 1 if fault == "los_p1" else 0
    chain = {}                                                                     # fault "no_reanchor": v carried across chunks
    for t0 in range(0, t_, kchunk):
        kmax = min(t_ - t0, kchunk)
        accx = np.zeros((kchunk, b_, ra, ta, p_), F)
        accy = np.zeros_like(accx)
        ca_prev = None
        for n in range(n_):
            ca, phi = draw(n)
            ts =F(t0 + (1 if fault == "restart_t0_plus_1" else 0)) / fs
            arg = (doppler * ts * ca + phi).astype(F)
            ca_w = ca_prev if (fault == "w_prev" and ca_prev is not None) else ca
            w = (doppler * (F(1) / fs) * ca_w).astype(F)
            ca_prev = ca
            sw, cw = np.sin(w), np.cos(w)
            if fault == "no_reanchor" and t0 > 0:
                vx, vy = chain[n]
            else:
                vx, vy = np.cos(arg), np.sin(arg)
            vx, vy = np.broadcast_to(vx, accx.shape[1:]).astype(F), np.broadcast_to(vy, accx.shape[1:]).astype(F)
            steps = kmax - 1 if (fault == "drop_last" and kmax < kchunk) else kmax
            for k in range(kchunk if fault == "no_reanchor" else steps):
                if k < steps:
                    accx[k] = accx[k] + vx
                    accy[k] = accy[k] + vy
                vx, vy = (vx * cw + (-vy) * sw).astype(F), (vy * cw + vx * sw).astype(F)
            if fault == "no_reanchor":
                chain[n] = (vx, vy)
        for k in range(kmax):
            t = t0 + k
            hx, hy = amp * (accx[k] * norm), amp * (accy[k] * norm)
            if los:
                cl = np.sin(F(los_aoa)) if fault == "los_sin" else np.cos(F(los_aoa))
                arg = (doppler[..., 0] * (F(t) / fs) * F(cl) + phi0).astype(F)
                kf = np.sqrt(F(los_power))
                hx[..., p_los] = hx[..., p_los] + np.cos(arg) * kf
                hy[..., p_los] = hy[..., p_los] + np.sin(arg) * kf
            out[..., t] = hx + 1j * hy
    return out[:, None, :, None]


def cdl_cir_model(tables, seed, call, batch, num_time_steps, sampling_frequency, min_speed, max_speed, fault=None):
    """Model of cdl_coupling_kernel + cdl_cir_kernel<float> in float32, operation for operation: ``tables`` are the float32 host
    tables of ``CDL._host_tables()``; the ray indices go through ``perm`` (stable ranks of the four key streams), the field chain
    is the kernel's expression, the rays are summed in ascending m, the LoS term last.  ``fault``: a seeded one-line fault
    (tests/test_tap_channel_host.py).  -> complex64 [B, 1, U, 1, S, N, T]"""
    from oracle import utils as outil
    f_rx, f_tx, a_rx, a_tx, r_rx, pol_rx, pol_tx, order, amp, los, xpr_scale, k0 = tables
    assert f_rx.dtype == F and a_rx.dtype == np.complex64
    b_, t_, rays = int(batch), int(num_time_steps), 20
    n_, u_, s_ = len(order), len(pol_rx), len(pol_tx)
    fs, k0, kx = F(sampling_frequency), F(k0), F(xpr_scale)
    if fault == "xpr_squared":
        kx = kx * kx
    v_r = _uni32(seed, call, b_, min_speed, max_speed)
    v_phi = _uni32(seed, call + 1, b_, 0, F(2) * PI_F)
    v_th = _uni32(seed, call + 2, b_, 0, PI_F)
    vx, vy, vz = v_r * np.cos(v_phi) * np.sin(v_th), v_r * np.sin(v_phi) * np.sin(v_th), v_r * np.cos(v_th)
    vx, vy, vz = (x.reshape(b_, 1) for x in (vx, vy, vz))
    perm = []
    for typ in range(4):                                                           # aoa, aod, zoa, zod
        keys = np.stack(outil.philox_block(seed, call + 3 + typ, (b_ * n_ * rays + 3) // 4), axis=1).reshape(-1)[:b_ * n_ * rays]
        perm.append(np.argsort(keys.reshape(b_, n_, rays), axis=-1, kind="stable"))
    ph = _uni32(seed, call + 7, b_ * n_ * rays * 4, -PI_F, PI_F).reshape(b_, n_, rays, 4)
    n_of = np.asarray(order)                                                       # cluster of output position no
    bi = np.arange(b_)[:, None]
    ps = np.zeros_like(pol_tx) if fault == "pol_tx_ignored" else pol_tx
    ampn = amp[np.arange(n_)] if fault == "amp_unordered" else amp[n_of]          # [No]
    ax = np.zeros((t_, b_, n_, u_, s_), F)
    ay = np.zeros_like(ax)
    tt = [F(t + (1 if fault == "time_plus_1" else 0)) / fs for t in range(t_)]

    def rotate(hr, hi, w):
        for t in range(t_):
            arg = (w * tt[t])[:, :, None, None]
            sn, cs = np.sin(arg), np.cos(arg)
            ax[t] += hr * cs - hi * sn
            ay[t] += hr * sn + hi * cs

    for m in range(rays):
        mz = (m + 1) % rays if fault == "zod_next_ray" else m
        ia, ja = perm[0][bi, n_of, m], perm[1][bi, n_of, m]                         # [B, No]
        iz, jz = perm[2][bi, n_of, m], perm[3][bi, n_of, mz]
        fr = f_rx[n_of, iz, ia][:, :, pol_rx]                                      # [B, No, U, 2]
        ft = f_tx[n_of, jz, ja][:, :, ps]                                          # [B, No, S, 2]
        frt, frp = fr[..., 0][..., None], fr[..., 1][..., None]
        ftt, ftp = ft[..., 0][:, :, None, :], ft[..., 1][:, :, None, :]
        e4 = ph[bi, n_of, m]                                                       # [B, No, 4]
        if fault == "phases_1_2_swapped":
            e4 = e4[..., [0, 2, 1, 3]]
        sn, cs = np.sin(e4)[:, :, None, None, :], np.cos(e4)[:, :, None, None, :]
        cr = frt * (cs[..., 0] * ftt + kx * cs[..., 1] * ftp) + frp * (kx * cs[..., 2] * ftt + cs[..., 3] * ftp)
        ci = frt * (sn[..., 0] * ftt + kx * sn[..., 1] * ftp) + frp * (kx * sn[..., 2] * ftt + sn[..., 3] * ftp)
        ar = a_rx[n_of, iz, ia][..., None]                                         # [B, No, U, 1]
        at = a_tx[n_of, jz, ja][:, :, None, :]
        if fault == "a_tx_conj":
            at = np.conj(at)
        gr, gi = ar.real * at.real - ar.imag * at.imag, ar.real * at.imag + ar.imag * at.real
        an = ampn[None, :, None, None]
        hr, hi = (cr * gr - ci * gi) * an, (cr * gi + ci * gr) * an
        rr = r_rx[n_of, jz, ja] if fault == "r_rx_departure" else r_rx[n_of, iz, ia]   # [B, No, 3]
        w = k0 * (rr[..., 0] * vx + rr[..., 1] * vy + rr[..., 2] * vz)
        rotate(hr, hi, w)
    if los is not None:
        frt, frp = los[0:4].reshape(2, 2)[pol_rx].T[:, :, None]                    # [U, 1] each
        ftt, ftp = los[4:8].reshape(2, 2)[ps].T[:, None, :]                        # [1, S]
        c = frt * ftt + frp * ftp if fault == "los_pm_identity" else frt * ftt - frp * ftp
        ar = los[8:8 + 2 * u_].reshape(u_, 2)[:, None, :]
        at = los[8 + 2 * u_:8 + 2 * u_ + 2 * s_].reshape(s_, 2)[None, :, :]
        if fault == "a_tx_conj":
            at = at * np.array([1, -1], F)
        rr = los[8 + 2 * u_ + 2 * s_:]
        kf = rr[3]
        gr = (ar[..., 0] * at[..., 0] - ar[..., 1] * at[..., 1]) * c * kf
        gi = (ar[..., 0] * at[..., 1] + ar[..., 1] * at[..., 0]) * c * kf
        w = k0 * (rr[0] * vx + rr[1] * vy + rr[2] * vz)                             # [B, 1]
        pos = 1 if fault == "los_position_1" else 0
        for t in range(t_):
            arg = (w * tt[t])[:, :, None]
            sn, cs = np.sin(arg), np.cos(arg)
            ax[t][:, pos] += gr * cs - gi * sn
            ay[t][:, pos] += gr * sn + gi * cs
    out = (ax + 1j * ay).astype(np.complex64)                                      # [T, B, No, U, S]
    return np.ascontiguousarray(np.transpose(out, [1, 3, 4, 2, 0]))[:, None, :, None]


# ------------------------------------------------------------------ LLR demappers (csrc/demap_core.h, csrc/mapping.hip)
_LOG2E_HI, _LOG2E_LO = np.uint32(0x3fb8aa3b).view(F), np.uint32(0x32a5705f).view(F)
_LN2_HI, _LN2_LO = np.uint32(0x3f317217).view(F), np.uint32(0x3377d1cf).view(F)
_TINY = np.finfo(F).tiny


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum rounds once more at 2^-53, far below float32"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def _hw_exp2(t):
    """v_exp_f32 stand-in: NumPy's float32 exp2; results below 2^-126 are returned as 0 (no denormal scaling)"""
    with np.errstate(under="ignore"):
        r = np.exp2(t.astype(F)).astype(F)
    return np.where(r < _TINY, F(0), r)


def _demap_exp(x, plain=False):
    x = x.astype(F)
    t = x * _LOG2E_HI
    if plain:
        return _hw_exp2(t)
    lo = _fma(x, _LOG2E_LO, _fma(x, _LOG2E_HI, -t))
    return _hw_exp2(t + lo)


def _exp_core(x):
    x = x.astype(F)
    t = x * _LOG2E_HI
    lo = _fma(x, _LOG2E_LO, _fma(x, _LOG2E_HI, -t))
    r = np.rint(t)
    f = (t - r) + lo
    with np.errstate(under="ignore"):
        return np.ldexp(np.exp2(f).astype(F), np.clip(r, -100000, 100000).astype(np.int32)).astype(F)


def _log_core(x):
    with np.errstate(divide="ignore"):
        y = np.log2(x.astype(F)).astype(F)
    r = y * _LN2_HI
    return r + _fma(y, _LN2_LO, _fma(y, _LN2_HI, -r))


def _bit_reduce(e, op):
    """bit_reduce<L> of demap_core.h on e [n, L]: r0 / r1 [n, NB], position p = label bit p (LSB = 0), the same tree"""
    L = e.shape[1]
    if L == 2:
        return e[:, :1].copy(), e[:, 1:2].copy()
    ev, od = e[:, 0], e[:, 1]
    for k in range(1, L // 2):
        ev, od = op(ev, e[:, 2 * k]), op(od, e[:, 2 * k + 1])
    r0, r1 = _bit_reduce(op(e[:, 0::2], e[:, 1::2]), op)
    return np.concatenate([ev[:, None], r0], axis=1), np.concatenate([od[:, None], r1], axis=1)


def _model_no(no, n, fault):
    no = np.asarray(no, F).reshape(-1)
    if no.size > 1 and fault == "neighbour_no":
        no = np.roll(no, -1)                     # the prefetched value of the next symbol
    if no.size > 1 and fault == "no0":
        no = no[:1]
    return np.broadcast_to(no, (n,))


def demap_square_model(y, no, levels, method, hard_out=False, threshold=64.0, fault=None):
    """``demap_square_qam_kernel`` / ``square_qam_llr``, operation by operation in float32: one reciprocal per symbol, the
    ``bit_reduce`` tree for maxima and sums, ``demap_exp`` with its extended-precision product and the flush of exponentials below
    2^-126, the switch to per-set maxima above ``threshold``.  y [n] complex64, no [1] or [n], levels [2^NB] -> [n, 2 NB]"""
    y = np.asarray(y, np.complex64).reshape(-1)
    lev = np.asarray(levels, F).copy()
    if fault == "level_4ulp":
        for _ in range(4):
            lev[0] = np.nextafter(lev[0], F(np.inf))
    n, L = y.size, len(lev)
    nb = int(np.log2(L))
    nv = _model_no(no, n, fault)
    ln2 = F(0.693147180559945)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        inv = F(1) / (nv if fault == "no_tiny" else np.maximum(nv, _TINY))
        llr = np.zeros((n, 2 * nb), F)
        for ax in range(2):
            ya = (y.imag if (ax == 0) == (fault == "axes_swapped") else y.real).astype(F)
            d = ya[:, None] - lev[None, :]
            e = -(d * d) * inv[:, None]
            mx0, mx1 = _bit_reduce(e, np.maximum)
            mall = np.maximum(mx0[:, nb - 1], mx1[:, nb - 1])
            if method == "app":
                ex = _demap_exp(e - mall[:, None], plain=fault == "plain_product")
                s0, s1 = _bit_reduce(ex, np.add)
            for t in range(nb):
                p = t if fault == "bit_order" else nb - 1 - t
                if method != "app":
                    llr[:, 2 * t + ax] = mx1[:, p] - mx0[:, p]
                    continue
                r = (np.log2(s1[:, p]) - np.log2(s0[:, p])).astype(F) * ln2
                if fault != "no_threshold":
                    a0, a1 = np.zeros(n, F), np.zeros(n, F)
                    for j in range(L):
                        if (j >> p) & 1:
                            a1 = a1 + _demap_exp(e[:, j] - mx1[:, p], plain=fault == "plain_product")
                        else:
                            a0 = a0 + _demap_exp(e[:, j] - mx0[:, p], plain=fault == "plain_product")
                    rb = (np.log2(a1).astype(F) * ln2 + mx1[:, p]) - (np.log2(a0).astype(F) * ln2 + mx0[:, p])
                    r = np.where(mall - np.minimum(mx0[:, p], mx1[:, p]) > F(threshold), rb, r)
                llr[:, 2 * t + ax] = r
    return (llr > 0).astype(F) if hard_out else llr


def demap_generic_model(y, no, points, method, prior=None, hard_out=False, fault=None):
    """``demap_kernel<M, MAXLOG>``: the IEEE division, pass 1 (per (bit, value) maxima), pass 2 (ascending-c sums of ``exp_core_f32``
    against the set's own maximum), ``log_core_f32``, the a-priori terms log_sigmoid(+-prior_i) summed over i from 0.
    y [n] complex64, no [1] or [n], points [2^m] complex64, prior None, [m] or [n, m] -> [n, m]"""
    y = np.asarray(y, np.complex64).reshape(-1)
    pts = np.asarray(points, np.complex64)
    n, P = y.size, len(pts)
    m = int(np.log2(P))
    nv = _model_no(no, n, fault)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        n0 = nv if fault == "no_tiny" else np.maximum(nv, _TINY)
        if prior is not None:
            p = np.broadcast_to(np.asarray(prior, F).reshape(-1, m), (n, m))
            p = -p if fault == "prior_sign" else p
            z_p, z_n = np.log1p(np.exp(p)).astype(F), np.log1p(np.exp(-p)).astype(F)
            ls1 = np.where(p < 0, p - z_p, -z_n).astype(F)
            ls0 = np.where(-p < 0, -p - z_n, -z_p).astype(F)

        def expo(c):
            dr, di = y.real.astype(F) - pts[c].real, y.imag.astype(F) - pts[c].imag
            e = -(dr * dr + di * di) / n0
            if prior is not None:
                ps = np.zeros(n, F)
                for i in range(m):
                    ps = ps + (ls1[:, i] if (c >> (m - 1 - i)) & 1 else ls0[:, i])
                e = ps + e
            return e.astype(F)

        ex = np.stack([expo(c) for c in range(P)], axis=1)                       # both passes recompute the same values
        bits = (np.arange(P)[:, None] >> np.arange(m - 1, -1, -1)) & 1          # [P, m]
        mx = np.stack([[np.max(ex[:, bits[:, i] == b], axis=1) for b in (0, 1)] for i in range(m)])        # [m, 2, n]
        if method != "app":
            llr = (mx[:, 1] - mx[:, 0]).T
        else:
            sm = np.zeros((m, 2, n), F)
            for c in range(P):
                for i in range(m):
                    b = bits[c, i]
                    sm[i, b] = sm[i, b] + _exp_core(ex[:, c] - mx[i, b] if fault == "no_clamp" else np.maximum(ex[:, c] - mx[i, b], F(-104)))
            llr = ((_log_core(sm[:, 1]) + mx[:, 1]) - (_log_core(sm[:, 0]) + mx[:, 0])).T
    llr = np.ascontiguousarray(llr, F)
    return (llr > 0).astype(F) if hard_out else llr


# ------------------------------------------------------------------ symbol-domain mapping kernels (csrc/mapping.hip)
def _f32_log_sigmoid(p, naive=False):
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        if naive:
            return np.log(F(1) / (F(1) + np.exp(-p).astype(F))).astype(F)
        return np.where(p < 0, p - np.log1p(np.exp(p).astype(F)).astype(F), -np.log1p(np.exp(-p).astype(F)).astype(F)).astype(F)


def _first_argmax_strict(e, last=False):
    """``if (e > mx) { mx = e; arg = c; }`` from -inf, arg = 0 (``last``: >=, the seeded fault)"""
    n, P = e.shape
    mx, arg = np.full(n, -np.inf, F), np.zeros(n, np.int32)
    for c in range(P):
        up = (e[:, c] >= mx) if last else (e[:, c] > mx)
        mx, arg = np.where(up, e[:, c], mx), np.where(up, c, arg).astype(np.int32)
    return mx, arg


def symbol_demap_model(y, no, points, prior=None, hard_out=False, fault=None):
    """``symbol_demap_kernel``: e_c = -(sqrtf(dr^2 + di^2))^2 / no (+ prior_c), strict first maximum, ascending sum of expf(e_c - mx),
    mx + logf(sum), e_c - lse.  y [n] complex64, no [1] or [n], points [P] complex64, prior None / [P] / [n, P] -> [n, P] (int32 [n])"""
    y = np.asarray(y, np.complex64).reshape(-1)
    pts = np.asarray(points, np.complex64)
    n, P = y.size, len(pts)
    nv = np.broadcast_to(np.asarray(no, F).reshape(-1), (n,))[:, None]
    with np.errstate(all="ignore"):
        dr, di = y.real.astype(F)[:, None] - pts.real[None, :], y.imag.astype(F)[:, None] - pts.imag[None, :]
        d = np.sqrt(dr * dr + di * di).astype(F)
        e = (-(d * d) / nv).astype(F)
        if prior is not None:
            e = (e + np.broadcast_to(np.asarray(prior, F).reshape(-1, P), (n, P))).astype(F)
        mx, arg = _first_argmax_strict(e, last=fault == "last_max")
        if hard_out:
            return arg
        sh = np.zeros(n, F) if fault == "no_shift" else mx
        s = np.zeros(n, F)
        for c in range(P - 1 if fault == "sum_pm1" else P):
            s = s + np.exp(e[:, c] - sh).astype(F)
        lse = sh + np.log(s).astype(F)
        return (e - lse[:, None]).astype(F)


def logits2llrs_model(z, m, method, prior=None, hard_out=False, fault=None):
    """``logits2llrs_kernel<M, MAXLOG>``: exponents = logits (+ sum_i log_sigmoid(+-prior_i) from 0), per (bit, value) maxima, ascending
    sums of ``exp_core_f32`` of the argument clamped at -104, ``log_core_f32`` + maximum - or the maximum itself where it is not finite
    (a whole set at -inf reduces to -inf, tf.reduce_logsumexp).  fault "unfixed": the kernel before the clamp and the empty-set rule"""
    z = np.asarray(z, F).reshape(-1, 1 << m)
    n, P = z.shape
    bits = (np.arange(P)[:, None] >> (np.arange(m) if fault == "lsb_first" else np.arange(m - 1, -1, -1))) & 1
    with np.errstate(all="ignore"):
        ex = z
        if prior is not None:
            p = np.asarray(prior, F).reshape(-1, m)
            p = np.broadcast_to(p[:1] if fault == "prior_as_vec" else p, (n, m))
            ls = np.stack([_f32_log_sigmoid(-p), _f32_log_sigmoid(p)], axis=-1)
            ex = np.zeros((n, P), F)
            for c in range(P):
                ps = np.zeros(n, F)
                for i in range(m):
                    ps = ps + ls[:, i, (c >> (m - 1 - i)) & 1]
                ex[:, c] = ps + z[:, c]
        mx = np.stack([[np.max(ex[:, bits[:, i] == b], axis=1) for b in (0, 1)] for i in range(m)])        # [m, 2, n]
        if method != "app":
            llr = (mx[:, 1] - mx[:, 0]).T
        else:
            sm = np.zeros((m, 2, n), F)
            for c in range(P):
                for i in range(m):
                    b = bits[c, i]
                    x = ex[:, c] - mx[i, b]
                    sm[i, b] = sm[i, b] + _exp_core(x if fault in ("unfixed", "unclamped") else np.maximum(x, F(-104)))
            r = _log_core(sm) + mx
            if fault not in ("unfixed", "no_empty_rule"):
                r = np.where(np.isfinite(mx), r, mx)
            llr = (r[:, 1] - r[:, 0]).T
    llr = np.ascontiguousarray(llr, F)
    return (llr > 0).astype(F) if hard_out else llr


def llrs2logits_model(llrs, m, hard_out=False, fault=None):
    """``llrs2logits_kernel``: the 2 m log-sigmoids of a row, then per point the sum over j from 0; hard_out: strict first maximum"""
    l = np.asarray(llrs, F).reshape(-1, m)
    n, P = l.shape[0], 1 << m
    ls = np.stack([_f32_log_sigmoid(-l, fault == "naive_log_sigmoid"), _f32_log_sigmoid(l, fault == "naive_log_sigmoid")], axis=-1)
    if fault == "sign_swapped":
        ls[:, 0] = ls[:, 0, ::-1]
    out = np.zeros((n, P), F)
    with np.errstate(all="ignore"):
        for c in range(P):
            acc = np.zeros(n, F)
            for j in range(m):
                acc = acc + ls[:, j, (c >> (m - 1 - j)) & 1]
            out[:, c] = acc
    return _first_argmax_strict(out, last=fault == "last_max")[1] if hard_out else out


def logits2moments_model(z, points, fault=None):
    """``logits2moments_kernel``: maximum, den = ascending sum of expf(z_c - mx), the weights expf(z_c - mx) / den formed again for the
    mean and again for the variance about the COMPUTED mean.  -> (mean complex64 [n], var float32 [n])"""
    pts = np.asarray(points, np.complex64)
    P = len(pts)
    z = np.asarray(z, F).reshape(-1, P)
    n = z.shape[0]
    xr, xi = pts.real.astype(F), pts.imag.astype(F)
    with np.errstate(all="ignore"):
        mx = z.max(-1) if n else np.zeros(0, F)
        den = np.zeros(n, F)
        for c in range(P):
            den = den + np.exp(z[:, c] - (F(0) if fault == "den_unshifted" else mx)).astype(F)
        mr, mi = np.zeros(n, F), np.zeros(n, F)
        for c in range(P - 1 if fault == "sum_pm1" else P):
            pc = np.exp(z[:, c] - mx).astype(F) / den
            mr, mi = mr + pc * xr[c], mi + pc * xi[c]
        v = np.zeros(n, F)
        for c in range(P):
            pc = np.exp(z[:, c] - mx).astype(F) / den
            if fault == "var_cancel":
                v = v + pc * (xr[c] * xr[c] + xi[c] * xi[c])
                continue
            dr, di = (xr[c] - mr, xi[c] - mi) if fault != "var_about_0" else (np.broadcast_to(xr[c], (n,)), np.broadcast_to(xi[c], (n,)))
            v = v + pc * (dr * dr + di * di)
        if fault == "var_cancel":
            v = v - (mr * mr + mi * mi)
    return (mr + 1j * mi).astype(np.complex64), v.astype(F)


def pam2qam_model(pam1, pam2, nbh, fault=None):
    """``pam2qam_logits_kernel``: out[i P + j] = pam1[t >> nbh] + pam2[t & (P - 1)], t = the interleaved label of (i, j)"""
    P = 1 << nbh
    a, b = np.asarray(pam1, F).reshape(-1, P), np.asarray(pam2, F).reshape(-1, P)
    out = np.zeros((a.shape[0], P * P), F)
    for i in range(P):
        for j in range(P):
            t = 0
            for k in range(nbh):
                t |= (((i >> (nbh - 1 - k)) & 1) << (2 * nbh - 1 - 2 * k)) | (((j >> (nbh - 1 - k)) & 1) << (2 * nbh - 2 - 2 * k))
            out[:, i * P + j] = a[:, i] + b[:, j] if fault == "scatter" else a[:, t >> nbh] + b[:, t & (P - 1)]
    return out
