"""Host-side code tables - mirror of reference src/sionna/phy/fec/conv/utils.py: ``polynomial_selector`` (:10-73) and
``Trellis`` (:76-190) in NumPy, with the same tables and attributes.  The kernels of csrc/conv.hip build the same trellis
from the generator polynomials (conv.hip ``build_trellis``)."""
import numpy as np

from ..utils import int2bin, bin2int


def polynomial_selector(rate, constraint_length):
    """Generator polynomials of [Moon] (best free distance) for rate 1/2 or 1/3 and constraint length 3..8
    (utils.py:10-73): a tuple of 0/1 strings."""
    if not isinstance(constraint_length, int):
        raise TypeError("constraint_length must be int.")
    if not 2 < constraint_length < 9:
        raise ValueError("Unsupported constraint_length.")
    if rate not in (1/2, 1/3):
        raise ValueError("Unsupported rate.")
    rate_half_dict = {3: ('101', '111'), 4: ('1101', '1011'), 5: ('10011', '11011'), 6: ('110101', '101111'),
                      7: ('1011011', '1111001'), 8: ('11100101', '10011111')}
    rate_third_dict = {3: ('101', '111', '111'), 4: ('1011', '1101', '1111'), 5: ('10101', '11011', '11111'),
                       6: ('100111', '101011', '111101'), 7: ('1111001', '1100101', '1011011'),
                       8: ('10010101', '11011001', '11110111')}
    return {1/2: rate_half_dict, 1/3: rate_third_dict}[rate][constraint_length]


def check_gen_poly(gen_poly, type_msg):
    """the reference's checks of a user ``gen_poly`` (encoding.py:113-121, decoding.py:113-121)"""
    if not all(isinstance(poly, str) for poly in gen_poly):
        raise TypeError(type_msg)
    if not all(len(poly) == len(gen_poly[0]) for poly in gen_poly):
        raise ValueError("Each polynomial must be of same length.")
    if not all(all(char in ['0', '1'] for char in poly) for poly in gen_poly):
        raise ValueError("Each polynomial must be a string of 0's and 1's.")


def select_gen_poly(rate, constraint_length):
    """the reference's checks of ``rate`` / ``constraint_length`` (encoding.py:123-132)"""
    if constraint_length not in (3, 4, 5, 6, 7, 8):
        raise ValueError("Constraint length must be between 3 and 8.")
    if rate not in (1/2, 1/3):
        raise ValueError("Rate must be 1/3 or 1/2.")
    return polynomial_selector(rate, constraint_length)


def kernel_code(gen_poly):
    """(polynomials as uint32 for the C-ABI, conv_n, constraint length); the kernels cover constraint lengths 3..8 and
    up to 8 polynomials"""
    L, n = len(gen_poly[0]), len(gen_poly)
    if not 3 <= L <= 8:
        raise ValueError(f"the convolutional-code kernels support constraint lengths 3..8 (gen_poly of length {L})")
    if not 1 <= n <= 8:
        raise ValueError(f"the convolutional-code kernels support 1..8 generator polynomials (got {n})")
    return np.array([int(p, 2) for p in gen_poly], np.uint32), n, L


class Trellis(object):
    """State transitions and output symbols of a rate-1/n convolutional code (utils.py:76-190).

    Attributes as in the reference, as int32 arrays: ``to_nodes`` [ns, 2] (state i, input j -> next state),
    ``from_nodes`` [ns, 2] (predecessors of state i, in the order the reference enumerates them), ``op_mat`` [ns, ns]
    (symbol emitted on i -> j, -1 if none), ``op_by_tonode`` / ``ip_by_tonode`` [ns, 2], ``op_by_fromnode`` [ns, 2]."""

    def __init__(self, gen_poly, rsc=True):
        self.rsc = rsc
        self.gen_poly = gen_poly
        self.constraint_length = len(self.gen_poly[0])
        self.conv_k = 1
        self.conv_n = len(self.gen_poly)
        self.ni = 2**self.conv_k
        self.ns = 2**(self.constraint_length-1)
        self._mu = len(gen_poly[0])-1
        if self.rsc:
            self.fb_poly = [int(x) for x in self.gen_poly[0]]
            assert self.fb_poly[0] == 1
            assert self.conv_k == 1
        self.to_nodes = None
        self.from_nodes = None
        self.op_mat = None
        self.op_by_tonode = None
        self.ip_by_tonode = None
        self._generate_transitions()

    def _binary_matmul(self, st):
        op = np.zeros(self.conv_n, int)
        assert len(st) == len(self.gen_poly[0])
        for i, poly in enumerate(self.gen_poly):
            op_int = sum(int(char)*int(poly[idx]) for idx, char in enumerate(st))
            op[i] = int2bin(op_int % 2, 1)[0]
        return op

    def _binary_vecmul(self, v1, v2):
        assert len(v1) == len(v2)
        op_int = sum(x*int(v2[idx]) for idx, x in enumerate(v1))
        return int2bin(op_int, 1)[0]

    def _generate_transitions(self):
        """utils.py:146-190: input i outer, current state j inner - this order fixes the order of ``from_nodes``"""
        ns, ni = self.ns, self.ni
        to_nodes = np.full((ns, ni), -1, int)
        from_nodes = np.full((ns, ni), -1, int)
        op_mat = np.full((ns, ns), -1, int)
        ip_by_tonode = np.full((ns, ni), -1, int)
        op_by_tonode = np.full((ns, ni), -1, int)
        op_by_fromnode = np.full((ns, ni), -1, int)
        from_nodes_ctr = np.zeros(ns, int)
        for i in range(ni):
            ip_bit = int2bin(i, self.conv_k)[0]
            for j in range(ns):
                curr_st_bits = int2bin(j, self.constraint_length-1)
                if self.rsc:
                    fb_bit = self._binary_vecmul(curr_st_bits, self.fb_poly[1:])
                    new_bit = int2bin(ip_bit + fb_bit, 1)[0]
                else:
                    new_bit = ip_bit
                state_bits = [new_bit] + curr_st_bits
                j_to = bin2int(state_bits[:-1])
                to_nodes[j][i] = j_to
                from_nodes[j_to][from_nodes_ctr[j_to]] = j
                op_sym = bin2int(self._binary_matmul(state_bits))
                op_mat[j, j_to] = op_sym
                op_by_tonode[j_to, from_nodes_ctr[j_to]] = op_sym
                ip_by_tonode[j_to, from_nodes_ctr[j_to]] = i
                op_by_fromnode[j][i] = op_sym
                from_nodes_ctr[j_to] += 1
        self.to_nodes = to_nodes.astype(np.int32)
        self.from_nodes = from_nodes.astype(np.int32)
        self.op_mat = op_mat.astype(np.int32)
        self.ip_by_tonode = ip_by_tonode.astype(np.int32)
        self.op_by_tonode = op_by_tonode.astype(np.int32)
        self.op_by_fromnode = op_by_fromnode.astype(np.int32)
