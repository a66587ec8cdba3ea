"""Specification (NumPy, CPU) of the RUNNING-TOTAL layered 5G LDPC decoder, min-sum family - the arithmetic
``csrc/ldpc5g_onchip_lyrt.hip`` is held to bit for bit (tests/test_gpu_layered_rt.py).

The reference's layered schedule (fec/ldpc/decoding.py:1383-1390: one sub-iteration per base row; _bp_iter with an array
schedule :463-520; vn_update_sum :681-732) updates the check nodes of a layer and then re-sums EVERY variable node over
all of its edges.  The textbook layered form keeps one running total per variable node instead and touches each edge once
per layer.  In exact arithmetic both are the same function; in floating point they differ by rounding, so this form has
its own definition - ONE sequence of IEEE operations, in the precision of ``dtype`` (float32: the kernel's; float64: the
anchor the closeness tests of tests/test_layered_rt_host.py compare against):

  initial state   xtot[v] = (-1 * clip(rate-recovered logit, -llr_max, llr_max)) + 0        (no -0 anywhere)
                  c[e]    = +0 for every edge (the message a check node sent last)
  per iteration, base rows ascending, per edge e = (check node, variable node v) of the row:
                  t      = xtot[v] - c[e]                  unclipped
                  v2c    = clip(t, -llr_max, llr_max)
                  c_new  = oracle.ldpc_bp.cn_update_minsum / cn_update_offset_minsum on the row's v2c
                           (sign convention of _sign_no_zero, output clip included)
                  xtot[v] = t + c_new[e];  c[e] = c_new[e]
  degree-1 variable nodes (the identity columns of the base graph's extension part): their total is llr + c, so
                  t = (llr + c) - c = llr in exact arithmetic.  The specification USES that identity: t = llr, never
                  the rounded difference, and xtot[v] = llr + c_new.
  output          x_hat = clip(xtot, -llr_max, llr_max) after the last layer, then the mapping of the existing decoder
                  (hard decision 0 >= x_hat or -1 * x_hat; return_infobits; shortened / punctured positions).

A base row holds at most one circulant per base column, so within a layer every variable node is touched by exactly one
check node: the order of the check nodes inside a layer does not matter (asserted below).

The kernel does not keep c[e] per edge.  For the min-sum family the messages a check node sends take at most two
magnitudes - one for the edge that delivered the unique minimum, one for all others - so a check node's record is
(a1, a2, word): a1 / a2 the smaller / larger SENT magnitude (after offset and output clip), bits 0..18 of the word the
sign bits of the sent messages, bits 24..28 the index of the edge that got a2 (the first one if several do, which only
happens when a1 == a2).  ``pack_records`` / ``unpack_records`` model that; ``check_packing=True`` asserts after every
layer that the record gives back c_new bit for bit.
"""
import numpy as np

from oracle import ldpc_bp as obp

IDX_SHIFT = 24


def pack_records(c_new):
    """c_new [checks, D, batch] (sent messages, edge order of the row) -> (a1, a2, word) of shape [checks, batch]."""
    d = c_new.shape[1]
    assert d <= 19
    mag = np.abs(c_new)
    a1, a2 = mag.min(axis=1), mag.max(axis=1)
    idx = np.argmax(mag, axis=1).astype(np.uint32)                     # first edge with the larger magnitude
    word = idx << np.uint32(IDX_SHIFT)
    for i in range(d):
        word = word | (np.signbit(c_new[:, i]).astype(np.uint32) << np.uint32(i))
    return a1, a2, word


def unpack_records(a1, a2, word, d):
    """the messages a record stands for, [checks, D, batch]"""
    out = np.empty((a1.shape[0], d) + a1.shape[1:], a1.dtype)
    idx = word >> np.uint32(IDX_SHIFT)
    for i in range(d):
        mag = np.where(idx == i, a2, a1)
        neg = ((word >> np.uint32(i)) & np.uint32(1)).astype(bool)
        out[:, i] = np.where(neg, -mag, mag)                          # (-0 for a negative zero magnitude, like the kernel's sign bit)
    return out


class LayeredRunningTotal(obp.LDPC5GDecoder):
    """oracle.ldpc_bp.LDPC5GDecoder(cn_schedule="layered") with the iteration loop replaced by the running-total form:
    pruning, rate recovery and the output mapping are the oracle's own code."""

    def __init__(self, code, cn_update="minsum", hard_out=True, return_infobits=True, num_iter=20, llr_max=20.,
                 precision="single", check_packing=False):
        if cn_update not in ("minsum", "min", "offset-minsum"):
            raise ValueError("the running-total specification covers the min-sum family")
        super().__init__(code, cn_update=cn_update, hard_out=hard_out, return_infobits=return_infobits, num_iter=num_iter,
                         llr_max=llr_max, precision=precision, cn_schedule="layered")
        self.check_packing = check_packing
        self.vn_of_cn_view = self.vn_idx[self.v2c_perm]                 # variable node of every edge, check-node view
        self.deg1 = self._vn_rag.deg == 1

    def decode(self, llr_ch, num_iter=None, msg_v2c=None):
        assert msg_v2c is None
        if num_iter is None:
            num_iter = self.num_iter
        dt = self.dtype
        llr_ch = np.asarray(llr_ch, dt)
        shape = llr_ch.shape
        llr = np.clip(llr_ch, -self.llr_max, self.llr_max).reshape(-1, self.num_vns).T.copy()
        llr = llr * dt(-1.) + dt(0.)                                    # [N_vn, B], no -0
        xtot = llr.copy()
        c = np.zeros((self.num_edges, llr.shape[1]), dt)                # check-node view order
        for _ in range(int(num_iter)):
            for pos, rag in self._sched:
                vn = self.vn_of_cn_view[pos]
                assert len(np.unique(vn)) == len(vn)                    # one check node per variable node and layer
                one = self.deg1[vn][:, None]
                t = np.where(one, llr[vn], xtot[vn] - c[pos]).astype(dt)
                v2c = np.clip(t, -self.llr_max, self.llr_max)
                c_new = self._cn_update(rag, v2c, self.llr_max).astype(dt)
                if self.check_packing:
                    d = len(pos) // rag.num_nodes                        # (the check nodes of a base row share its degree)
                    cn3 = c_new.reshape(rag.num_nodes, d, -1)
                    back = unpack_records(*pack_records(cn3), d)
                    assert np.array_equal(back.view(np.uint32 if dt == np.float32 else np.uint64),
                                          cn3.view(np.uint32 if dt == np.float32 else np.uint64)), "record does not give c_new back"
                xtot[vn] = t + c_new
                c[pos] = c_new
        x_hat = np.clip(xtot, -self.llr_max, self.llr_max).T
        x_hat = (0 >= x_hat).astype(dt) if self.hard_out else x_hat * dt(-1.)
        return x_hat.reshape(shape[:-1] + (self.num_vns,))
