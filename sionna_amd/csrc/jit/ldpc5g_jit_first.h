// Item bodies of the lean FIRST iteration of the specialised 5G LDPC decoder (min-sum / offset-min-sum, no state): source TEXT
// like ldpc5g_jit_templates.h, appended behind it only in the programs whose first trip is lean (csrc/ldpc5g_jit_gen.cpp:
// Class1Emitter::lean_first) - every other program keeps its text.  Written against the same per-lane operations, so
// tests/jit_emu compiles them.

// ---- the first iteration (min-sum / offset-min-sum): the channel value of a punctured column is +0 on every lane, so a row
// with such an edge, at index PE, has m1 = 0 and sends magnitude 0 on every edge but PE - and a variable node that adds +-0 to
// its sum and subtracts it again returns its channel value, which init() already stored.  What is left of the row's update is
// the ONE message to edge PE.  jit_cn_update's output for edge PE with v_PE = +0: |v_PE| == m1 = 0 selects a2;
// min_e = (m2 - 0) + 0 = m2, the smallest magnitude of the OTHER edges (with multiplicity: a second zero gives m2 = 0); the
// clip of min-sum is the identity because every v2c was clipped by its sender, m2 <= llr_max; offset-min-sum clips m2 - offset
// as there.  The sign: v_PE = +0 adds nothing to the row's parity, and mag ^ (v_PE & msb) = mag.  Hence: the minimum of |v|
// over all edges but PE (the fused column's channel value lf included, from registers), the parity of their signs, one store.
// The slot of edge PE is never read: it holds the previous codeword's message.
template <int D, int NCH, bool FUSE, int PE>
JIT_DEV void jit_cn_first(U32 a0, const F32 (&lf)[NCH], float llr_max, float offset) {
  F32 v[D][NCH];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (i == PE) continue;
    if (FUSE && i == D - 1) {
#pragma unroll
      for (int h = 0; h < NCH; ++h) v[i][h] = lf[h];
    } else if (JIT_LAYOUT_B && NCH == 2) lds_ld2(a0, (unsigned)i * JIT_Z4, v[i][0], v[i][NCH - 1]);
    else {
#pragma unroll
      for (int h = 0; h < NCH; ++h) v[i][h] = lds_ld(a0, (unsigned)i * JIT_Z4 + JIT_CH * h);
    }
  }
  F32 c2v[NCH];
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    F32 m = f_abs(v[PE == 0 ? 1 : 0][h]);
    U32 sx = 0u;
#pragma unroll
    for (int k = 0; k < D - 1; ++k) {                    // k-th of the D - 1 edges that are not PE
      const int i = k < PE ? k : k + 1, ip = (k - 1) < PE ? k - 1 : k;
      if (k >= 1) m = f_med3(m, f_abs(v[i][h]), 0.f);
      if (k & 1) sx = u_xor3(sx, f_bits(v[ip][h]), f_bits(v[i][h]));
      else if (k == D - 2) sx = sx ^ f_bits(v[i][h]);
    }
    const F32 a = JIT_OFFSET0 ? m : f_med3(m - offset, 0.f, llr_max);
    c2v[h] = u_float(f_bits(a) | (sx & 0x80000000u));
  }
  jit_cn_store<NCH>(a0, (unsigned)PE * JIT_Z4, c2v);
}

// ---- the first iteration, variable node of a punctured column (channel value +0): the c2v of the HAVE edges come from rows
// whose only zero-magnitude input this column is (jit_cn_first); every other edge carries +-0, which neither changes the sum
// (a partial sum is never -0: it starts from +0, +0 + -0 = +0, exact cancellation rounds to +0) nor the difference x - c.  So:
// the sum over the HAVE edges in edge order, plus l; v2c = clip(x - c) on the HAVE edges and clip(x) on the others; every edge is
// stored, only the HAVE edges are loaded - the other slots hold the previous codeword's messages.
template <int D, unsigned HAVE>
JIT_DEV void jit_vnb_first(const U32 (&a)[D], const M64 (&sw)[D], const F32 (&l)[2], float llr_max) {
  F32 x0 = 0.f, x1 = 0.f;
  F32 v0[D], v1[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (!((HAVE >> i) & 1u)) continue;
    F32 c0, c1;
    lds_ld2(a[i], 0u, c0, c1);
    v0[i] = f_sel(sw[i], c1, c0);                        // slot order -> node order
    v1[i] = f_sel(sw[i], c0, c1);
    f_pk_add(x0, x1, v0[i], v1[i]);
  }
  f_pk_add(x0, x1, l[0], l[1]);
  const F32 y0 = f_med3(x0, -llr_max, llr_max), y1 = f_med3(x1, -llr_max, llr_max);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    F32 e0 = y0, e1 = y1;
    if ((HAVE >> i) & 1u) {
      f_pk_sub(e0, e1, x0, x1, v0[i], v1[i]);
      e0 = f_med3(e0, -llr_max, llr_max);
      e1 = f_med3(e1, -llr_max, llr_max);
    }
    lds_st2(a[i], 0u, f_sel(sw[i], e1, e0), f_sel(sw[i], e0, e1));    // node order -> slot order
  }
}
template <int D, int NCH, unsigned HAVE>
JIT_DEV void jit_vn_first(const U32 (&a)[D][NCH], const F32 (&l)[NCH], float llr_max) {
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    F32 c[D];
    F32 x = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (!((HAVE >> i) & 1u)) continue;
      c[i] = lds_ld(a[i][h], 0u);
      x = x + c[i];
    }
    x = x + l[h];
    const F32 y = f_med3(x, -llr_max, llr_max);
#pragma unroll
    for (int i = 0; i < D; ++i) lds_st(a[i][h], 0u, ((HAVE >> i) & 1u) ? f_med3(x - c[i], -llr_max, llr_max) : y);
  }
}
