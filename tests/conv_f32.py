"""Specification of the convolutional-code kernels (csrc/conv.hip): the reference's ConvEncoder, ViterbiDecoder and
BCJRDecoder (src/sionna/phy/fec/conv/encoding.py:221-292, decoding.py:236-453, 700-943) restated in NumPy float32 /
float64 in the kernels' order of operations.

Orders the reference leaves open, fixed here (and in the kernels):
  - branch metrics: the conv_n terms summed in index order ((v0 + v1) + v2 ...);
  - sums over the ns states of a codeword (the map normalisation, the two LLR sums of map, the exp sums of the log-sum-exp
    over states): the halving fold x[:h] + x[h:] until one value is left;
  - exp / log in float32: the float64 function rounded once to float32 (np.exp(x.astype(float64)).astype(float32)).
Viterbi and BCJR maxlog involve only IEEE add, compare and sign changes: the kernels are bit-identical to this file.  map and
log call exp / log; the kernels' float64 exp / log are within 1 ulp of NumPy's, so the float32 results agree except where
the float64 value lies within an ulp of a float32 rounding boundary (conv row, states the bar)."""
import numpy as np

from sionna_amd.phy.fec.conv.utils import Trellis

LARGEDIST = 2.**20


def _exp(x):
    return np.exp(x.astype(np.float64)).astype(x.dtype) if x.dtype == np.float32 else np.exp(x)


def _log(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.astype(np.float64)).astype(x.dtype) if x.dtype == np.float32 else np.log(x)


def fold_sum(x):
    """halving fold over the last axis (length a power of two)"""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def lse_states(x):
    """tf.reduce_logsumexp over the last axis: max (replaced by 0 when not finite), fold sum of exp(x - max), log + max"""
    m = np.max(x, axis=-1)
    m = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    with np.errstate(invalid="ignore"):
        return _log(fold_sum(_exp(x - m[..., None]))) + m


def lse2(a, b):
    m = np.maximum(a, b)
    m = np.where(np.isfinite(m), m, 0).astype(a.dtype)
    with np.errstate(invalid="ignore"):
        return _log(_exp(a - m) + _exp(b - m)) + m


def out_bits(conv_n):
    """[2^conv_n, conv_n]: bits of output symbol o, the first polynomial's bit first (int2bin)"""
    o = np.arange(2**conv_n)[:, None]
    return (o >> np.arange(conv_n - 1, -1, -1)[None, :]) & 1


def encode(u, gen_poly, rsc=False, terminate=False):
    """u [B, k] 0/1 -> codeword [B, conv_n (k + mu terminate)] uint8 (the trellis walk of encoding.py:250-290)"""
    tr = Trellis(gen_poly, rsc=rsc)
    u = np.asarray(u).astype(np.int64) & 1
    B, k = u.shape
    mu, cn = tr._mu, tr.conv_n
    st = np.zeros(B, np.int64)
    bits = out_bits(cn)
    out = []
    for t in range(k + (mu if terminate else 0)):
        if t < k:
            i = u[:, t]
        elif rsc:                                                   # feed the feedback bit: register input 0
            i = np.array([tr.to_nodes[s][1] >> (mu - 1) == 0 for s in st], np.int64)
        else:
            i = np.zeros(B, np.int64)
        new = tr.to_nodes[st, i]
        out.append(bits[tr.op_mat[st, new]])
        st = new
    return np.concatenate(out, axis=1).astype(np.uint8) if out else np.zeros((B, 0), np.uint8)


def viterbi(y, gen_poly, rsc=False, terminate=False, method="soft_llr", return_info_bits=True, dtype=np.float32):
    """y [B, n] -> [B, k] information bits (or [B, n] codeword bits along the path), dtype 0/1"""
    tr = Trellis(gen_poly, rsc=rsc)
    cn, mu, ns = tr.conv_n, tr._mu, tr.ns
    y = np.asarray(y, dtype)
    B, n = y.shape
    T = n // cn
    k = T - (mu if terminate else 0)
    Y = y.reshape(B, T, cn)
    if method == "hard":
        r = np.abs(np.rint(Y))
        Y = (r - dtype(2) * np.floor(r / dtype(2))).astype(dtype)
    ob = out_bits(cn).astype(dtype)                                 # [no, cn]
    acc = None
    for j in range(cn):                                             # [B, T, no], summed in index order
        b = ob[None, None, :, j]
        v = np.abs(Y[..., j:j + 1] - b) if method == "hard" else np.where(b == 1, -Y[..., j:j + 1], Y[..., j:j + 1])
        acc = v if acc is None else acc + v
    bm = acc.astype(dtype)
    cm = np.full((B, ns), LARGEDIST, dtype)
    cm[:, 0] = 0
    dec = np.zeros((T, B, ns), bool)
    f0, f1 = tr.from_nodes[:, 0], tr.from_nodes[:, 1]
    o0, o1 = tr.op_by_tonode[:, 0], tr.op_by_tonode[:, 1]
    for t in range(T):
        m0 = cm[:, f0] + bm[:, t, o0]
        m1 = cm[:, f1] + bm[:, t, o1]
        d = m1 < m0                                                 # argmin: the first minimum
        cm = np.where(d, m1, m0)
        dec[t] = d
    cur = np.zeros(B, np.int64) if terminate else np.argmin(cm, axis=1)
    ar = np.arange(B)
    u = np.zeros((B, T), dtype)
    c = np.zeros((B, T, cn), dtype)
    bits = out_bits(cn)
    for t in range(T - 1, -1, -1):
        prev = tr.from_nodes[cur, dec[t, ar, cur].astype(np.int64)] if t > 0 else np.zeros(B, np.int64)
        m0 = tr.to_nodes[prev, 0] == cur
        m1 = tr.to_nodes[prev, 1] == cur
        u[:, t] = m1
        sym = np.where(m0, tr.op_by_fromnode[prev, 0], np.where(m1, tr.op_by_fromnode[prev, 1], 0))
        c[:, t] = bits[sym]
        cur = prev
    return u[:, :k] if return_info_bits else c.reshape(B, n)


def bcjr(llr_ch, gen_poly, rsc=False, terminate=False, algorithm="map", hard_out=True, llr_a=None, dtype=np.float32):
    """llr_ch [B, n], llr_a [B, T] or None -> [B, k] LLRs log p(1)/p(0) or hard decisions"""
    tr = Trellis(gen_poly, rsc=rsc)
    cn, mu, ns = tr.conv_n, tr._mu, tr.ns
    y = np.asarray(llr_ch, dtype)
    B, n = y.shape
    T = n // cn
    k = T - (mu if terminate else 0)
    la = np.zeros((B, T), dtype) if llr_a is None else np.asarray(llr_a, dtype).reshape(B, T)
    yn, lan = -y, -la                                               # log p(0)/p(1) internally (decoding.py:924-925)
    Y = yn.reshape(B, T, cn)
    ob = out_bits(cn)
    acc = None
    for j in range(cn):                                             # bm [B, T, no] = sum_j 0.5 (llr_j (1 - 2 c_j))
        b = ob[None, None, :, j]
        v = dtype(0.5) * np.where(b == 1, -Y[..., j:j + 1], Y[..., j:j + 1])
        acc = v if acc is None else acc + v
    bm = acc.astype(dtype)
    h = dtype(0.5) * lan                                            # signed half a priori LLR: b = 0 -> +h, b = 1 -> -h
    sl = np.stack([h, -h], axis=-1)                                 # [B, T, 2]
    mapa = algorithm == "map"
    if mapa:
        bm, sl = _exp(bm), _exp(sl)
    one, zero = (dtype(1), dtype(0)) if mapa else (dtype(0), dtype(-np.inf))
    alpha = np.full((B, ns), zero, dtype)
    alpha[:, 0] = one
    if terminate:
        beta = alpha.copy()
    else:
        eq = 1. / ns
        beta = np.full((B, ns), eq if mapa else np.log(eq), dtype)

    def gamma(t, b, o):                                             # [B, ns]
        return sl[:, t, b] * bm[:, t, o] if mapa else sl[:, t, b] + bm[:, t, o]

    def comb(a, b):
        if mapa:
            return a + b
        return lse2(a, b) if algorithm == "log" else np.maximum(a, b)

    alphas = np.zeros((T, B, ns), dtype)
    f, ip, op = tr.from_nodes, tr.ip_by_tonode, tr.op_by_tonode
    for t in range(T):
        alphas[t] = alpha
        term = []
        for j in range(2):
            g = gamma(t, ip[:, j], op[:, j])
            p = alpha[:, f[:, j]]
            term.append(g * p if mapa else g + p)
        na = comb(term[0], term[1])
        if mapa:
            na = na / fold_sum(na)[:, None]
        alpha = na.astype(dtype)
    to, of = tr.to_nodes, tr.op_by_fromnode
    llr = np.zeros((B, T), dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            at = alphas[t]
            g = [gamma(t, np.full(ns, b), of[:, b]) for b in range(2)]
            bb = [beta[:, to[:, b]] for b in range(2)]
            if mapa:
                nb = g[0] * bb[0] + g[1] * bb[1]
                nb = nb / fold_sum(nb)[:, None]
                l0 = (at * g[0]) * bb[0]
                l1 = (at * g[1]) * bb[1]
                llr[:, t] = _log(fold_sum(l0) / fold_sum(l1))
            else:
                nb = comb(g[0] + bb[0], g[1] + bb[1])
                l0 = (at + g[0]) + bb[0]
                l1 = (at + g[1]) + bb[1]
                if algorithm == "log":
                    llr[:, t] = lse_states(l0) - lse_states(l1)
                else:
                    llr[:, t] = np.max(l0, axis=-1) - np.max(l1, axis=-1)
            beta = nb.astype(dtype)
    m = -llr[:, :k]
    return (dtype(0) < m).astype(dtype) if hard_out else m


def llr_bar(llr_ch, llr_a=None):
    """agreement bar of map / log against this file (per codeword): 1e-5 (1 + sum |llr_ch| + sum |llr_a|) - the log
    domain metrics grow with the sum of the codeword's |LLR|, and a 1-ulp difference of one exp / log is carried at that
    magnitude"""
    s = np.sum(np.abs(np.asarray(llr_ch, np.float64)), axis=-1)
    if llr_a is not None:
        s = s + np.sum(np.abs(np.asarray(llr_a, np.float64)), axis=-1)
    return 1e-5 * (1 + s)
