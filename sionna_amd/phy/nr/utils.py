"""5G NR helpers of the transport-block chain - mirror of reference src/sionna/phy/nr/utils.py
(``generate_prng_seq`` :14-78, ``decode_mcs_index`` :80-304, ``calculate_num_coded_bits`` :374-471,
``calculate_tb_size`` :473-805).  Scalar arguments (the TB blocks only need scalars); init-time host arithmetic in the
reference's float32."""
import functools

import numpy as np
import torch

from ... import _ffi

# 38.214 Table 5.1.3.2-1
_TAB51321 = np.array([-1, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128, 136, 144, 152, 160, 168, 176, 184, 192,
                      208, 224, 240, 256, 272, 288, 304, 320, 336, 352, 368, 384, 408, 432, 456, 480, 504, 528, 552, 576,
                      608, 640, 672, 704, 736, 768, 808, 848, 888, 928, 984, 1032, 1064, 1128, 1160, 1192, 1224, 1256,
                      1288, 1320, 1352, 1416, 1480, 1544, 1608, 1672, 1736, 1800, 1864, 1928, 2024, 2088, 2152, 2216,
                      2280, 2408, 2472, 2536, 2600, 2664, 2728, 2792, 2856, 2976, 3104, 3240, 3368, 3496, 3624, 3752,
                      3824], np.float32)


def generate_prng_seq(length, c_init):
    """38.211 Sec. 5.2.1 length-31 Gold sequence as a NumPy array of 0/1 floats (utils.py:14-78);
    produced by ``samd_nr_prng_seq_f32``."""
    assert length % 1 == 0 and int(length) > 0, "length must be a positive integer."
    assert c_init % 1 == 0, "c_init must be integer."
    assert 0 <= int(c_init) < 2 ** 32, "c_init must be in [0, 2^32-1]."
    out = torch.empty(int(length), dtype=torch.float32, device=_ffi.device())
    _ffi.check(_ffi.lib().samd_nr_prng_seq_f32(int(c_init), int(length), _ffi.ptr(out), _ffi.stream()),
               "generate_prng_seq")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=256)
def _prng_seq_host(length, c_init):
    """the same sequence on the host, int8 and read-only: c(n) = x1(n + 1600) + x2(n + 1600) mod 2 with
    x1(n + 31) = x1(n + 3) + x1(n), x2(n + 31) = x2(n + 3) + x2(n + 2) + x2(n + 1) + x2(n), x1 = 1, x2 = c_init at the start
    (38.211 Sec. 5.2.1).  The configuration objects build the DMRS from it without a device."""
    assert 0 <= int(c_init) < 2 ** 32 and int(length) > 0
    total = int(length) + 1600
    x1, x2 = np.zeros(total + 31, np.int8), np.zeros(total + 31, np.int8)
    x1[0] = 1
    x2[:31] = (int(c_init) >> np.arange(31)) & 1
    for i in range(total):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    c = x1[1600:total] ^ x2[1600:total]
    c.setflags(write=False)
    return c


# 38.214 Tables 6.1.4.1-1 / -2 (PUSCH with transform precoding; the entries that depend on q are written for q = 1) and
# 5.1.3.1-1 .. -4: modulation order and target code rate x 1024 per MCS index, -1 where the index is reserved
_MCS_ORDER = np.array([
    [[1] * 2 + [2] * 8 + [4] * 7 + [6] * 11 + [-1],
     [1] * 6 + [2] * 10 + [4] * 8 + [6] * 4 + [-1],
     [-1] * 29,
     [-1] * 29],
    [[2] * 10 + [4] * 7 + [6] * 12,
     [2] * 5 + [4] * 6 + [6] * 9 + [8] * 8 + [-1],
     [2] * 15 + [4] * 6 + [6] * 8,
     [2] * 3 + [4] * 3 + [6] * 9 + [8] * 8 + [10] * 4 + [-1] * 2]], np.int32)
_MCS_RATE = np.array([
    [[240, 314, 193, 251, 308, 379, 449, 526, 602, 679, 340, 378, 434, 490, 553, 616, 658, 466, 517, 567, 616, 666, 719, 772,
      822, 873, 910, 948, -1],
     [60, 80, 100, 128, 156, 198, 120, 157, 193, 251, 308, 379, 449, 526, 602, 679, 378, 434, 490, 553, 616, 658, 699, 772,
      567, 616, 666, 772, -1],
     [-1] * 29,
     [-1] * 29],
    [[120, 157, 193, 251, 308, 379, 449, 526, 602, 679, 340, 378, 434, 490, 553, 616, 658, 438, 466, 517, 567, 616, 666, 719,
      772, 822, 873, 910, 948],
     [120, 193, 308, 449, 602, 378, 434, 490, 553, 616, 658, 466, 517, 567, 616, 666, 719, 772, 822, 873, 682.5, 711, 754,
      797, 841, 885, 916.5, 948, -1],
     [30, 40, 50, 64, 78, 99, 120, 157, 193, 251, 308, 379, 449, 526, 602, 340, 378, 434, 490, 553, 616, 438, 466, 517, 567,
      616, 666, 719, 772],
     [120, 193, 449, 378, 490, 616, 466, 517, 567, 616, 666, 719, 772, 822, 873, 682.5, 711, 754, 797, 841, 885, 916.5, 948,
      805.5, 853, 900.5, 948, -1, -1]]], np.float32)


def decode_mcs_index(mcs_index, table_index=1, is_pusch=True, transform_precoding=False, pi2bpsk=False,
                     check_index_validity=True, verbose=False):
    """Modulation order (int32) and target code rate (float32) of an MCS index, 38.214 Sec. 5.1.3.1 / 6.1.4.1
    (utils.py:80-304).  Scalars or arrays of one shape; NumPy values, since the configuration objects live on the host."""
    mcs_index = np.asarray(mcs_index).astype(np.int32)
    shape = mcs_index.shape

    def shaped(v, dtype):
        v = np.asarray(v)
        assert v.shape in ((), shape), "inconsistent input shapes"
        return np.broadcast_to(v.astype(dtype), shape)

    table_index = shaped(table_index, np.int32)
    is_pusch, transform_precoding, pi2bpsk = shaped(is_pusch, bool), shaped(transform_precoding, bool), shaped(pi2bpsk, bool)
    assert np.all(mcs_index >= 0), "MCS index cannot be negative"
    assert np.all(mcs_index <= 28), "MCS index cannot be higher than 28"
    assert np.all(np.isin(table_index, [1, 2, 3, 4])), "table_index must contain values in [1,2,3,4]"
    if verbose:
        print(f"Selected MCS index {mcs_index} for {np.where(is_pusch, 'PUSCH', 'PDSCH')} channel and Table index {table_index}.")
    # row 0: PUSCH with transform precoding; row 1: PDSCH, and PUSCH without it
    row = (~is_pusch | ~transform_precoding).astype(np.int32)
    order = _MCS_ORDER[row, table_index - 1, mcs_index]
    rate = _MCS_RATE[row, table_index - 1, mcs_index]
    if check_index_validity and np.any(order < 0):
        raise ValueError("Invalid MCS index")
    # tp-pi2BPSK: q = 1, else q = 2, on the first entries of the two transform-precoding tables
    on_q = (row == 0) & (((table_index == 1) & (mcs_index < 2)) | ((table_index == 2) & (mcs_index < 6)))
    q = np.where(pi2bpsk, 1, 2).astype(np.int32)
    order = np.where(on_q, order * q, order).astype(np.int32)
    rate = (np.where(on_q, rate / q.astype(np.float32), rate) / np.float32(1024)).astype(np.float32)
    if verbose:
        print(f"Modulation order: {order}")
        print(f"Target code rate: {rate}")
    return order[()], rate[()]


def calculate_num_coded_bits(modulation_order, num_prbs, num_ofdm_symbols, num_dmrs_per_prb, num_layers=1, num_ov=0,
                             tb_scaling=1.0, precision=None):
    """Coded bits that fit into a slot (utils.py:374-471)."""
    assert 1 <= num_ofdm_symbols <= 14, "num_ofdm_symbols must be in [1, 14]."
    assert 1 <= num_prbs <= 275, "num_prbs must be in [1, 275]."
    assert tb_scaling in (0.25, 0.5, 1.0), "tb_scaling must be 0.25, 0.5, or 1.0."
    n_re_per_prb = min(156, 12 * int(num_ofdm_symbols) - int(num_dmrs_per_prb) - int(num_ov))
    return int(np.float32(tb_scaling) * np.float32(n_re_per_prb * int(num_prbs) * int(modulation_order) * int(num_layers)))


def calculate_tb_size(modulation_order, target_coderate, target_tb_size=None, num_coded_bits=None, num_prbs=None,
                      num_ofdm_symbols=None, num_dmrs_per_prb=None, num_layers=1, num_ov=0, tb_scaling=1.0,
                      return_cw_length=True, verbose=False, precision=None):
    """Transport block size of 38.214 Sec. 5.1.3.2 / 6.1.4.2 (utils.py:473-805).
    Returns ``(tb_size, cb_size, num_cb, tb_crc_length, cb_crc_length[, cw_length])``."""
    f = np.float32
    if num_coded_bits is None:
        assert num_prbs is not None and num_ofdm_symbols is not None and num_dmrs_per_prb is not None, \
            "If num_coded_bits is None then num_prbs, num_ofdm_symbols, num_dmrs_per_prb must be specified."
        num_coded_bits = calculate_num_coded_bits(modulation_order, num_prbs, num_ofdm_symbols, num_dmrs_per_prb,
                                                  num_layers, num_ov, tb_scaling)
    num_coded_bits, num_layers, modulation_order = int(num_coded_bits), int(num_layers), int(modulation_order)
    assert num_coded_bits % num_layers == 0, "num_coded_bits must be a multiple of num_layers."
    if target_tb_size is not None:
        t = f(target_tb_size)
        assert t < f(num_coded_bits), "target_tb_size must be less than num_coded_bits."
    else:
        t = f(target_coderate) * f(num_coded_bits)
    if t <= 3824:
        n = max(f(3.0), f(np.floor(np.log(t) / f(np.log(2.0))) - 6))
        n_info_q = max(f(24.0), f(f(2) ** n * np.floor(t / f(2) ** n)))
    else:
        n = np.floor(np.log(t - f(24)) / np.log(f(2.0))) - f(5.)
        n_info_q = max(f(3840.0), f(f(2) ** n * np.round((t - f(24)) / f(2) ** n)))
    if n_info_q <= 3824:
        num_cb = 1
        ge = _TAB51321 >= n_info_q
        ind = int(np.argmax(np.cumsum(1 - 2 * ge.astype(np.float32))))
        tb_size = int(_TAB51321[min(ind + 1, len(_TAB51321) - 1)])
    else:
        if target_coderate <= 1 / 4:
            num_cb = int(np.ceil((n_info_q + f(24)) / f(3816)))
        elif n_info_q > 8424:
            num_cb = int(np.ceil((n_info_q + f(24)) / f(8424)))
        else:
            num_cb = 1
        tb_size = int(f(8) * f(num_cb) * np.ceil((n_info_q + f(24)) / (f(8) * f(num_cb))) - f(24))
    tb_crc_length = 24 if tb_size > 3824 else 16
    cb_crc_length = 24 if num_cb > 1 else 0
    cb_size = int((tb_size + tb_crc_length) / num_cb) + cb_crc_length
    if verbose:
        print(f"Modulation order: {modulation_order}")
        if target_coderate is not None:
            print(f"Target coderate: {target_coderate:.3f}")
        print(f"Effective coderate: {tb_size / num_coded_bits:.3f}")
        print(f"Number of layers: {num_layers}")
        print("------------------")
        print(f"Info bits per TB: {tb_size}")
        print(f"TB CRC length: {tb_crc_length}")
        print(f"Total number of coded TB bits: {num_coded_bits}")
        print("------------------")
        print(f"Info bits per CB: {cb_size}")
        print(f"Number of CBs: {num_cb}")
        print(f"CB CRC length: {cb_crc_length}")
    if not return_cw_length:
        return tb_size, cb_size, num_cb, tb_crc_length, cb_crc_length
    q = num_layers * modulation_order
    num_last = int(num_coded_bits / q) % num_cb
    len_last = q * int(np.ceil(num_coded_bits / (q * num_cb)))
    len_first = q * int(np.floor(num_coded_bits / (q * num_cb)))
    cw_length = np.array([len_first] * (num_cb - num_last) + [len_last] * num_last, np.int64)
    return tb_size, cb_size, num_cb, tb_crc_length, cb_crc_length, cw_length
