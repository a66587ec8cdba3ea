"""Specification of the PUSCH grid kernel (csrc/pusch.hip) in NumPy, float32 and float64.

    grid[b, tx, l, re] = points[label(bits[b, tx, (d * L + l) * m : (d * L + l) * m + m])]   d = data_pos[tx * L + l, re] >= 0
                       = pilots[tx * L + l, p]                                               p = pilot_pos[tx * L + l, re] >= 0
                       = 0                                                                   otherwise
    out[b, tx, q, re]  = sum_{l = 0..L-1} w[tx, q, l] * grid[b, tx, l, re]                   (w None: out = grid)

The label of m bits is their value read most significant bit first; L is the number of layers, so the bit index is the
mapper and the layer mapper in one.  Every port's real and imaginary part start at +0 and add, in ascending l,
(wr * xr - wi * xi) and (wr * xi + wi * xr): four products, one difference, one sum, and the two accumulations, each rounded
once to ``dtype``.

``separate_blocks`` is the composition the fused evaluation must equal: mapper, layer mapper, grid mapper, precoder."""
import numpy as np


def _cdtype(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def mapper(bits, points, m):
    """[..., n] 0/1 -> [..., n / m] constellation points"""
    bits = np.asarray(bits)
    b = bits.reshape(bits.shape[:-1] + (-1, m)).astype(np.int64)
    return points[(b << np.arange(m - 1, -1, -1)).sum(-1)]


def layer_mapper(x, num_layers):
    """[..., n] -> [..., num_layers, n / num_layers]: symbol i goes to layer i mod num_layers"""
    return np.swapaxes(x.reshape(x.shape[:-1] + (-1, num_layers)), -1, -2)


def grid_mapper(x, pilots, data_pos, pilot_pos):
    """x [B, num_tx, L, num_data] -> [B, num_tx, L, num_re]; the tables are [num_tx * L, num_re]"""
    b, num_tx, num_layers, _ = x.shape
    xs = x.reshape(b, num_tx * num_layers, -1)
    out = np.zeros((b,) + data_pos.shape, x.dtype)
    for s in range(data_pos.shape[0]):
        has_data, has_pilot = data_pos[s] >= 0, (data_pos[s] < 0) & (pilot_pos[s] >= 0)
        out[:, s, has_data] = xs[:, s, data_pos[s][has_data]]
        if pilots.shape[-1]:
            out[:, s, has_pilot] = pilots[s, pilot_pos[s][has_pilot]]
    return out.reshape(b, num_tx, num_layers, -1)


def precoder(grid, w, dtype=np.float32):
    """grid [B, num_tx, L, num_re], w [num_tx, P, L] -> [B, num_tx, P, num_re] in the kernel's order of operations"""
    w = np.asarray(w).astype(_cdtype(dtype))
    xr, xi = grid.real.astype(dtype), grid.imag.astype(dtype)
    wr, wi = w.real[None, :, :, :, None], w.imag[None, :, :, :, None]
    shape = grid.shape[:2] + (w.shape[1], grid.shape[3])
    ar, ai = np.zeros(shape, dtype), np.zeros(shape, dtype)
    for l in range(grid.shape[2]):
        a, b = xr[:, :, l:l + 1], xi[:, :, l:l + 1]
        ar = ar + (wr[:, :, :, l] * a - wi[:, :, :, l] * b)
        ai = ai + (wr[:, :, :, l] * b + wi[:, :, :, l] * a)
    assert ar.dtype == dtype
    out = np.empty(shape, _cdtype(dtype))
    out.real, out.imag = ar, ai
    return out


def separate_blocks(bits, points, pilots, data_pos, pilot_pos, w, num_layers, dtype=np.float32):
    cd = _cdtype(dtype)
    points, pilots = np.asarray(points).astype(cd), np.asarray(pilots).astype(cd)
    m = int(np.log2(len(points)))
    grid = grid_mapper(layer_mapper(mapper(bits, points, m), num_layers), pilots, data_pos, pilot_pos)
    return grid if w is None else precoder(grid, w, dtype)


def pusch_grid(bits, points, pilots, data_pos, pilot_pos, w, num_layers, dtype=np.float32):
    """bits [B, num_tx, num_data * L * m] -> [B, num_tx, P, num_re] through ONE evaluation of the formula: the label of
    every (layer, resource element) is read at its bit index, no intermediate tensor is laid out"""
    cd = _cdtype(dtype)
    bits = np.asarray(bits)
    points, pilots = np.asarray(points).astype(cd), np.asarray(pilots).astype(cd)
    m, L = int(np.log2(len(points))), num_layers
    b, num_tx, _ = bits.shape
    grid = np.zeros((b, num_tx, L, data_pos.shape[1]), cd)
    weights = 1 << np.arange(m - 1, -1, -1)
    for tx in range(num_tx):
        for l in range(L):
            s = tx * L + l
            re = np.nonzero(data_pos[s] >= 0)[0]
            first = (data_pos[s][re].astype(np.int64) * L + l) * m
            label = (bits[:, tx][:, first[:, None] + np.arange(m)].astype(np.int64) * weights).sum(-1)
            grid[:, tx, l, re] = points[label]
            pil = np.nonzero((data_pos[s] < 0) & (pilot_pos[s] >= 0))[0]
            if pilots.shape[-1]:
                grid[:, tx, l, pil] = pilots[s, pilot_pos[s][pil]]
    return grid if w is None else precoder(grid, w, dtype)


def error_bound(points64, pilots64, data_pos, pilot_pos, w64, bits, num_layers, unit=2.0 ** -24, dtype=np.float32):
    """Per output and real component (float64 array [B, num_tx, P, num_re]): what ``pusch_grid`` in ``dtype`` may differ by from
    the exact value of the formula on the float64 constellation, pilots and matrices.
        (L + 3) * unit * sum_l |w_l| |x_l|  +  sum_l |w_l| |fl(c_l) - c_l|
    With x the value a layer carries and |.| the complex modulus, a real component of w x is wr xr - wi xi with
    |wr xr| + |wi xi| <= |w| |x|.  Roundings: one per product (unit |w| |x| together), one for the difference or sum of the two
    products, L - 1 for the accumulation (the first addition, to +0, is exact), one for w stored in ``dtype`` and one for a
    pilot stored in ``dtype``: L + 3 units of sum_l |w_l| |x_l|.  A constellation point c is normalised in ``dtype`` by the
    mapping module, more than one rounding, so its distance to the float64 point is measured and added.  Without
    precoding w is the identity."""
    cd = _cdtype(dtype)
    L = num_layers
    g64 = pusch_grid(bits, points64, pilots64, data_pos, pilot_pos, None, L, np.float64)
    dpoints = np.asarray(points64).astype(cd).astype(np.complex128)
    delta = np.abs(pusch_grid(bits, dpoints, np.zeros_like(pilots64), data_pos, pilot_pos, None, L, np.float64)
                   - pusch_grid(bits, points64, np.zeros_like(pilots64), data_pos, pilot_pos, None, L, np.float64))
    if w64 is None:
        w_abs = np.broadcast_to(np.eye(L)[None], (g64.shape[1], L, L))
    else:
        w_abs = np.abs(np.asarray(w64))
    scale = np.einsum("tql,btlr->btqr", w_abs, np.abs(g64))
    return (L + 3) * unit * scale + np.einsum("tql,btlr->btqr", w_abs, delta)
