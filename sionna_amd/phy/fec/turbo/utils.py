"""Utilities of the turbo codes - mirror of reference src/sionna/phy/fec/turbo/utils.py: ``polynomial_selector`` (:10-46),
``puncture_pattern`` (:49-78) and ``TurboTermination`` (:81-296), and ``turbo_tables``, the index tables through which the
kernels of csrc/turbo.hip read and write a punctured turbo codeword."""
import math

import numpy as np
import torch

from ...block import Object


def polynomial_selector(constraint_length):
    """Generator polynomials of the rate-1/2 recursive systematic constituent code for constraint length 3..6
    (utils.py:10-46): a tuple of two 0/1 strings, the first the feedback polynomial."""
    if not isinstance(constraint_length, int):
        raise TypeError("constraint_length must be int.")
    if not 2 < constraint_length < 7:
        raise ValueError("Unsupported constraint_length.")
    gen_poly_dict = {
        3: ('111', '101'),          # (7, 5)
        4: ('1011', '1101'),        # (13, 15)
        5: ('10011', '11011'),      # (23, 33)
        6: ('111101', '101011'),    # (75, 53)
    }
    return gen_poly_dict[constraint_length]


def puncture_pattern(turbo_coderate, conv_coderate):
    """Boolean pattern [periods, 3] of the bits kept of (systematic, parity 1, parity 2) so that the turbo code has rate
    ``turbo_coderate`` over constituent codes of rate ``conv_coderate`` = 1/2 (utils.py:49-78)."""
    if conv_coderate != 1/2:
        raise ValueError("conv_coderate must be 1/2.")
    if turbo_coderate == 1/2:
        pattern = [[1, 1, 0], [1, 0, 1]]
    elif turbo_coderate == 1/3:
        pattern = [[1, 1, 1]]
    else:
        raise NotImplementedError("turbo_coderate not supported")
    return torch.tensor(pattern, dtype=torch.bool)


class TurboTermination(Object):
    """``TurboTermination(constraint_length, conv_n=2, num_conv_encs=2, num_bitstreams=3)`` (utils.py:81-296): where the
    termination bits of the two constituent encoders sit in the turbo codeword.  Works on NumPy arrays and on tensors."""

    def __init__(self, constraint_length, conv_n=2, num_conv_encs=2, num_bitstreams=3, **kwargs):
        super().__init__(**kwargs)
        constraint_length = int(constraint_length)
        conv_n = int(conv_n)
        num_conv_encs = int(num_conv_encs)
        num_bitstreams = int(num_bitstreams)
        self.mu_ = constraint_length - 1
        self.conv_n = conv_n
        if num_conv_encs != 2:
            raise NotImplementedError("Only num_conv_encs=2 supported.")
        self.num_conv_encs = num_conv_encs
        self.num_bitstreams = num_bitstreams

    def get_num_term_syms(self):
        """Number of termination symbols of the turbo code, one symbol being ``num_bitstreams`` bits (utils.py:133-154)"""
        total_term_bits = self.conv_n * self.num_conv_encs * self.mu_
        return math.ceil(total_term_bits/self.num_bitstreams)

    def termbits_conv2turbo(self, term_bits1, term_bits2):
        """[..., conv_n mu] termination bits of encoder 1 and of encoder 2 -> [..., num_bitstreams num_term_syms]: the two
        concatenated, zero-padded on the right to a whole number of turbo symbols (utils.py:156-230)"""
        is_np = not isinstance(term_bits1, torch.Tensor)
        a, b = torch.as_tensor(term_bits1), torch.as_tensor(term_bits2)
        term_bits = torch.cat([a, b.to(a.device)], dim=-1)
        num_term_bits = term_bits.shape[-1]
        extra_bits = self.num_bitstreams * math.ceil(num_term_bits/self.num_bitstreams) - num_term_bits
        if extra_bits > 0:
            term_bits = torch.nn.functional.pad(term_bits, (0, extra_bits))
        return term_bits.numpy() if is_np else term_bits

    def term_bits_turbo2conv(self, term_bits):
        """[..., 3 num_term_syms] termination part of a turbo codeword -> the [..., conv_n mu] parts of encoder 1 and of
        encoder 2 (utils.py:232-295)"""
        if term_bits.shape[-1] % self.num_bitstreams != 0:
            raise ValueError("Programming Error.")
        m = self.conv_n * self.mu_
        return term_bits[..., :m], term_bits[..., m:2*m]


def turbo_tables(k, coderate, terminate, mu, perm):
    """Index tables of a turbo codeword of ``k`` information bits, NumPy int32, for the kernels of csrc/turbo.hip.

    The unpunctured codeword is k + S rows of (systematic, parity 1, parity 2), S = ceil(4 mu / 3) termination rows when
    ``terminate`` holding the 2 mu termination bits of encoder 1, those of encoder 2 and zero padding
    (fec/turbo/utils.py:156-230); rate 1/2 keeps (1, 1, 0) of the even and (1, 0, 1) of the odd rows, a last incomplete
    period included (encoding.py:291-341, decoding.py:340-355).  Returns a dict:
      n      codeword bits after puncturing
      T      trellis steps of a constituent code, k + mu when terminated
      idx1   [T, 2] position in the codeword of (systematic, parity) of step t of decoder 1, -1 punctured
      idx2   [T, 2] the same for decoder 2; its systematic values are those of decoder 1 interleaved
      opos   [2, T, 2] where encoder e writes the output bits of step t: idx1 and idx2, but the systematic bits of
             encoder 2 before the termination are not transmitted (-1)
      zpos   [2] positions of the zero padding that survive the puncturing, -1 none
      perm, inv  [k] the interleaver and its inverse."""
    k, mu = int(k), int(mu)
    perm = np.asarray(perm, np.int64)
    if perm.shape != (k,) or not np.array_equal(np.sort(perm), np.arange(k)):
        raise ValueError("the interleaver is not a permutation of 0..k-1")
    S = math.ceil(4 * mu / 3) if terminate else 0
    rows = k + S
    if coderate == 1/3:
        mask = np.ones((rows, 3), bool)
    elif coderate == 1/2:
        mask = np.where((np.arange(rows) % 2 == 0)[:, None], [True, True, False], [True, False, True])
    else:
        raise NotImplementedError("turbo_coderate not supported")
    mask = mask.reshape(-1)
    pos = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int64)       # unpunctured position -> codeword position
    n = int(mask.sum())
    T = k + (mu if terminate else 0)
    t = np.arange(k)
    idx1 = np.full((T, 2), -1, np.int64)
    idx2 = np.full((T, 2), -1, np.int64)
    idx1[:k, 0], idx1[:k, 1] = pos[3 * t], pos[3 * t + 1]
    idx2[:k, 0], idx2[:k, 1] = pos[3 * perm], pos[3 * t + 2]
    zpos = np.full(2, -1, np.int64)
    if terminate:
        i = np.arange(mu)
        base = 3 * k
        idx1[k:, 0], idx1[k:, 1] = pos[base + 2 * i], pos[base + 2 * i + 1]
        idx2[k:, 0], idx2[k:, 1] = pos[base + 2 * mu + 2 * i], pos[base + 2 * mu + 2 * i + 1]
        pad = pos[base + 4 * mu:3 * rows]
        pad = pad[pad >= 0]
        zpos[:len(pad)] = pad
    opos = np.stack([idx1, idx2])
    opos[1, :k, 0] = -1
    inv = np.argsort(perm, kind="stable")
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return {"n": n, "T": T, "idx1": i32(idx1), "idx2": i32(idx2), "opos": i32(opos), "zpos": i32(zpos),
            "perm": i32(perm), "inv": i32(inv)}
