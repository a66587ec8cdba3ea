"""``PUSCHConfig`` - a physical uplink shared channel, 38.211 Sec. 6.3 / 6.4 (mirror of reference
src/sionna/phy/nr/pusch_config.py:12-1065): symbol allocation, the DMRS positions of Tables 6.4.1.1.3-3 / -4, the DMRS grid
of Sec. 6.4.1.1.3, the codebook of Tables 6.3.1.5-1 .. -7, and the slot's number of coded bits and transport-block size.
Host-side NumPy; the Gold sequence is ``utils._prng_seq_host`` so that no device is needed."""
import numpy as np

from .carrier_config import CarrierConfig
from .config import Config
from .pusch_dmrs_config import PUSCHDMRSConfig
from .tb_config import TBConfig
from .utils import _prng_seq_host, calculate_tb_size

# Additional DMRS positions l_bar after l_0, Tables 6.4.1.1.3-3 (single-symbol) and -4 (double-symbol):
# (shortest duration l_d the row applies from, positions for dmrs-AdditionalPosition 1, 2, 3).  Below the first row of a
# table no DMRS symbol is defined at all.
_L_BAR = {
    ("A", 1): [(4, ((), (), ())), (8, ((7,), (7,), (7,))), (10, ((9,), (6, 9), (6, 9))), (12, ((9,), (6, 9), (5, 8, 11))),
               (13, ((11,), (7, 11), (5, 8, 11)))],
    ("A", 2): [(4, ((),)), (10, ((8,),)), (13, ((10,),))],
    ("B", 1): [(0, ((), (), ())), (5, ((4,), (4,), (4,))), (8, ((6,), (3, 6), (3, 6))), (10, ((8,), (4, 8), (3, 6, 9))),
               (12, ((10,), (5, 10), (3, 6, 9)))],
    ("B", 2): [(5, ((),)), (8, ((5,),)), (10, ((7,),)), (12, ((9,),))],
}

# Precoding matrices W of Tables 6.3.1.5-1 .. -7 by (layers, antenna ports): per TPMI the rows of W, one character per
# entry (1, 0, - = -1, j, k = -j), and the number W is divided by.
_ENTRY = {"1": 1, "0": 0, "-": -1, "j": 1j, "k": -1j}
_S2, _S3 = np.sqrt(2), np.sqrt(3)
_ONE_LAYER_FOUR_PORTS = ("1000111100001111111111111111", "0100000011111111jjjj----kkkk", "00101-jk00001j-k1j-k1j-k1j-k",
                         "000100001-jk1j-kj-k1-k1jk1j-")
_CODEBOOK = {
    (1, 2): [(w, _S2) for w in ("1 0", "0 1", "1 1", "1 -", "1 j", "1 k")],
    (1, 4): [(" ".join(row[i] for row in _ONE_LAYER_FOUR_PORTS), 2) for i in range(28)],
    (2, 2): [("10 01", _S2), ("11 1-", 2), ("11 jk", 2)],
    (2, 4): [(w, 2) for w in ("10 01 00 00", "10 00 01 00", "10 00 00 01", "00 10 01 00", "00 10 00 01", "00 00 10 01",
                              "10 01 10 0k", "10 01 10 0j", "10 01 k0 01", "10 01 k0 0-", "10 01 -0 0k", "10 01 -0 0j",
                              "10 01 j0 01", "10 01 j0 0-")] +
            [(w, 2 * _S2) for w in ("11 11 1- 1-", "11 11 jk jk", "11 jj 1- jk", "11 jj jk -1", "11 -- 1- -1", "11 -- jk kj",
                                    "11 kk 1- kj", "11 kk jk 1-")],
    (3, 4): [(w, 2) for w in ("100 010 001 000", "100 010 100 001", "100 010 -00 001")] +
            [(w, 2 * _S3) for w in ("111 1-1 11- 1--", "111 1-1 jjk jkk", "111 -1- 11- -11", "111 -1- jjk kjj")],
    (4, 4): [("1000 0100 0010 0001", 2), ("1100 0011 1-00 001-", 2 * _S2), ("1100 0011 jk00 00jk", 2 * _S2),
             ("1111 1-1- 11-- 1--1", 4), ("1111 1-1- jjkk jkkj", 4)],
}


class PUSCHConfig(Config):
    def __init__(self, carrier_config=None, pusch_dmrs_config=None, tb_config=None, **kwargs):
        super().__init__(**kwargs)
        self._name = "PUSCH Configuration"
        self.carrier = carrier_config
        self.dmrs = pusch_dmrs_config
        self.tb = tb_config
        self.check_config()

    # ---- children
    @property
    def carrier(self):
        return self._carrier

    @carrier.setter
    def carrier(self, value):
        if value is None:
            value = CarrierConfig()
        assert isinstance(value, CarrierConfig), "carrier must be an instance of CarrierConfig"
        self._carrier = value

    @property
    def dmrs(self):
        return self._dmrs

    @dmrs.setter
    def dmrs(self, value):
        if value is None:
            value = PUSCHDMRSConfig()
        assert isinstance(value, PUSCHDMRSConfig), "pusch_dmrs_config must be an instance of PUSCHDMRSConfig"
        self._dmrs = value

    @property
    def tb(self):
        return self._tb

    @tb.setter
    def tb(self, value):
        if value is None:
            value = TBConfig(channel_type="PUSCH")
        assert isinstance(value, TBConfig), "tb must be an instance of TBConfig"
        assert value.channel_type == "PUSCH", 'TBConfig must be configured for "PUSCH"'
        self._tb = value

    # ---- configurable
    @property
    def n_size_bwp(self):
        self._ifndef("n_size_bwp", None)
        return self._n_size_bwp

    @n_size_bwp.setter
    def n_size_bwp(self, value):
        if value is not None:
            assert value in range(1, 276), "n_size_bwp must be in the range from 1 to 275"
        self._n_size_bwp = value

    @property
    def n_start_bwp(self):
        self._ifndef("n_start_bwp", 0)
        return self._n_start_bwp

    @n_start_bwp.setter
    def n_start_bwp(self, value):
        assert value in range(0, 2474), "n_start_bwp must be in the range from 0 to 2473"
        self._n_start_bwp = value

    @property
    def num_layers(self):
        self._ifndef("num_layers", 1)
        return self._num_layers

    @num_layers.setter
    def num_layers(self, value):
        assert value in [1, 2, 3, 4], "num_layers must be in [1,...,4]"
        self._num_layers = value

    @property
    def num_antenna_ports(self):
        self._ifndef("num_antenna_ports", 1)
        return self._num_antenna_ports

    @num_antenna_ports.setter
    def num_antenna_ports(self, value):
        assert value in [1, 2, 4], "num_antenna_ports must be in [1,2,4]"
        self._num_antenna_ports = value

    @property
    def mapping_type(self):
        self._ifndef("mapping_type", "A")
        return self._mapping_type

    @mapping_type.setter
    def mapping_type(self, value):
        assert value in ["A", "B"], "mapping_type must be A or B"
        self._mapping_type = value

    @property
    def symbol_allocation(self):
        self._ifndef("symbol_allocation", [0, 14])
        return self._symbol_allocation

    @symbol_allocation.setter
    def symbol_allocation(self, value):
        assert len(value) == 2, "symbol_allocation must have two elements"
        self._symbol_allocation = value

    @property
    def n_rnti(self):
        self._ifndef("n_rnti", 1)
        return self._n_rnti

    @n_rnti.setter
    def n_rnti(self, value):
        if value is not None:
            assert value in range(65536), "n_rnti must be in [0, 65535]"
        self._n_rnti = value

    @property
    def precoding(self):
        self._ifndef("precoding", "non-codebook")
        return self._precoding

    @precoding.setter
    def precoding(self, value):
        assert value in ["codebook", "non-codebook"], "Unknown value for precoding"
        self._precoding = value

    @property
    def transform_precoding(self):
        self._ifndef("transform_precoding", False)
        return self._transform_precoding

    @transform_precoding.setter
    def transform_precoding(self, value):
        assert isinstance(value, bool), "transform_precoding must be bool"
        self._transform_precoding = value

    @property
    def tpmi(self):
        self._ifndef("tpmi", 0)
        return self._tpmi

    @tpmi.setter
    def tpmi(self, value):
        assert value in range(28), "tpmi must be in [0,...,27]"
        self._tpmi = value

    # ---- read-only
    @property
    def frequency_hopping(self):
        return "neither"

    @property
    def l_0(self):
        """first DMRS symbol relative to l_ref"""
        return self.dmrs.type_a_position if self.mapping_type == "A" else 0

    @property
    def l_d(self):
        return self.symbol_allocation[1]

    @property
    def l_ref(self):
        return 0 if self.mapping_type == "A" else self.symbol_allocation[0]

    @property
    def l_prime(self):
        return list(range(self.dmrs.length))

    @property
    def l_bar(self):
        """first symbols of the DMRS positions (Tables 6.4.1.1.3-3 / -4)"""
        extra = None
        for l_d_min, per_position in _L_BAR[(self.mapping_type, self.dmrs.length)]:
            if self.l_d >= l_d_min:
                extra = per_position
        if extra is None:
            return []
        pos = self.dmrs.additional_position
        return [self.l_0] + (list(extra[pos - 1]) if pos > 0 else [])

    @property
    def l(self):
        return [l_bar + l_prime for l_bar in self.l_bar for l_prime in self.l_prime]

    @property
    def n(self):
        per_n = 4 if self.dmrs.config_type == 1 else 6
        return list(range(self.num_subcarriers // per_n))

    @property
    def dmrs_symbol_indices(self):
        return [l + self.l_ref for l in self.l]

    @property
    def num_resource_blocks(self):
        return self.carrier.n_size_grid if self.n_size_bwp is None else self.n_size_bwp

    @property
    def num_subcarriers(self):
        return 12 * self.num_resource_blocks

    @property
    def num_res_per_prb(self):
        """resource elements of a PRB that carry data: all of a data symbol, and of a DMRS symbol those outside the CDM
        groups without data (6 subcarriers per group with configuration type 1, 4 with type 2)"""
        num_dmrs = len(self.dmrs_symbol_indices)
        per_group = 6 if self.dmrs.config_type == 1 else 4
        return (self.symbol_allocation[1] - num_dmrs) * 12 + num_dmrs * (12 - per_group * self.dmrs.num_cdm_groups_without_data)

    def _cdm_group_subcarriers(self, group):
        """subcarriers of one PRB that CDM group ``group`` occupies"""
        if self.dmrs.config_type == 1:
            return np.arange(group, 12, 2)
        return np.array([0, 1, 6, 7]) + 2 * group

    @property
    def dmrs_mask(self):
        """[num_subcarriers, num_symbols_per_slot] bool: resource elements that carry no data"""
        mask = np.zeros([self.num_subcarriers, self.carrier.num_symbols_per_slot], dtype=bool)
        prb = 12 * np.arange(self.num_resource_blocks)[:, None]
        for group in range(self.dmrs.num_cdm_groups_without_data):
            sc = (prb + self._cdm_group_subcarriers(group)[None, :]).reshape(-1)
            mask[np.ix_(sc, self.dmrs_symbol_indices)] = True
        return mask

    @property
    def dmrs_grid(self):
        """[num_dmrs_ports, num_subcarriers, num_symbols_per_slot] complex: the unprecoded DMRS of every port,
            a(k, l) = beta w_f(k') w_t(l') r(2 n + k'),   k = 4 n + 2 k' + Delta (type 1) or 6 n + k' + Delta (type 2),
        with r the QPSK sequence of Sec. 6.4.1.1.1.1 seeded per symbol by ``c_init``"""
        self.check_config()
        dmrs = self.dmrs
        ports = dmrs.dmrs_port_set if len(dmrs.dmrs_port_set) > 0 else list(range(self.num_layers))
        saved, dmrs.dmrs_port_set = dmrs.dmrs_port_set, ports
        try:
            w_f, w_t, deltas = dmrs.w_f, dmrs.w_t, dmrs.deltas
        finally:
            dmrs.dmrs_port_set = saved
        a_tilde = np.zeros([len(ports), self.num_subcarriers, self.carrier.num_symbols_per_slot], dtype=complex)
        n = np.asarray(self.n)
        for l_bar in self.l_bar:
            for l_prime in self.l_prime:
                l = l_bar + l_prime
                c = _prng_seq_host(2 * self.num_subcarriers, self.c_init(l)).astype(np.float64)
                r = 1 / np.sqrt(2) * ((1 - 2 * c[::2]) + 1j * (1 - 2 * c[1::2]))
                for j in range(len(ports)):
                    for k_prime in (0, 1):
                        if dmrs.config_type == 1:
                            k = 4 * n + 2 * k_prime + deltas[j]
                        else:
                            k = 6 * n + k_prime + deltas[j]
                        a_tilde[j, k, self.l_ref + l] = r[2 * n + k_prime] * w_f[k_prime][j] * w_t[l_prime][j]
        return dmrs.beta * a_tilde

    @property
    def dmrs_grid_precoded(self):
        """[num_antenna_ports, num_subcarriers, num_symbols_per_slot]: W applied to the DMRS ports (None without codebook)"""
        if self.precoding == "non-codebook":
            return None
        a = np.transpose(self.dmrs_grid, [1, 2, 0])[..., None]
        return np.transpose(np.matmul(self.precoding_matrix[None, None], a)[..., 0], [2, 0, 1])

    @property
    def precoding_matrix(self):
        """[num_antenna_ports, num_layers] complex: W of the configured TPMI; None without codebook precoding"""
        if self.precoding == "non-codebook" or self.num_antenna_ports == 1:
            return None
        table = _CODEBOOK.get((self.num_layers, self.num_antenna_ports))
        if table is None:
            return None
        rows, divisor = table[self.tpmi]
        w = np.array([[_ENTRY[ch] for ch in row] for row in rows.split()], complex)
        w /= divisor
        return w

    @property
    def num_ov(self):
        return 0

    @property
    def num_coded_bits(self):
        n_re = (self.num_res_per_prb - self.num_ov) * self.num_resource_blocks
        return int(self.tb.tb_scaling * self.tb.num_bits_per_symbol * self.num_layers * n_re)

    @property
    def tb_size(self):
        """information bits of a slot: at most 156 resource elements per PRB count (38.214 Sec. 6.1.4.2); the product is
        formed in float64 from the float32 code rate, then quantised by ``calculate_tb_size``"""
        n_re = min(156, self.num_res_per_prb - self.num_ov) * self.num_resource_blocks
        target = int(float(self.tb.target_coderate) * self.tb.tb_scaling * n_re * int(self.tb.num_bits_per_symbol) * self.num_layers)
        return calculate_tb_size(target_tb_size=target, num_coded_bits=self.num_coded_bits,
                                 target_coderate=self.tb.target_coderate, modulation_order=self.tb.num_bits_per_symbol,
                                 verbose=False)[0]

    def c_init(self, l):
        """seed of the DMRS sequence of OFDM symbol ``l`` (Sec. 6.4.1.1.1.1, lambda_bar = 0)"""
        n_scid = self.dmrs.n_scid
        n_id = self.carrier.n_cell_id if self.dmrs.n_id is None else self.dmrs.n_id[n_scid]
        symbol = self.carrier.num_symbols_per_slot * self.carrier.slot_number + l + 1
        return int((2 ** 17 * symbol * (2 * n_id + 1) + 2 * n_id + n_scid) % 2 ** 31)

    def show(self):
        self.carrier.show()
        Config.show(self)
        self.dmrs.show()
        self.tb.show()

    def check_config(self):
        self.carrier.check_config()
        self.dmrs.check_config()
        alloc, dmrs = self.symbol_allocation, self.dmrs
        if self.precoding == "codebook":
            if len(dmrs.dmrs_port_set) > 0:
                assert len(dmrs.dmrs_port_set) == self.num_layers, "num_layers must be equal to the number of dmrs ports"
            assert self.num_layers <= self.num_antenna_ports, "num_layers must be <= num_antenna_ports"
            assert self.num_antenna_ports >= 2, "precoding requires two or more antenna ports"
        else:
            assert self.num_layers == self.num_antenna_ports, "num_layers must be == num_antenna_ports"
        # the rows of Tables 6.4.1.1.3-3 / -4 that exist
        if dmrs.length == 1:
            if self.mapping_type == "A":
                assert alloc[1] >= 4, "Symbol allocation is too short"
        else:
            assert dmrs.additional_position < 2, "dmrs.additional_position must be <2 for this dmrs.length"
            assert alloc[1] >= 4, "Symbol allocation too short"
            if self.mapping_type == "B":
                assert alloc[1] >= 5, "Symbol allocation is too short"
        if self.mapping_type == "A" and dmrs.additional_position == 3:
            assert dmrs.type_a_position == 2, "additional_position=3 only allowed for type_a_position=2"
        # the TPMI must index the table of (layers, ports)
        table = _CODEBOOK.get((self.num_layers, self.num_antenna_ports))
        num_tpmi = len(table) if table is not None else {3: 7, 4: 5}.get(self.num_layers)
        if num_tpmi is not None:
            assert self.tpmi in range(num_tpmi), f"tpmi must be in [0,...,{num_tpmi - 1}]"
        max_length = 14 if self.carrier.cyclic_prefix == "normal" else 12
        if self.mapping_type == "A":
            assert alloc[0] == 0, "symbol_allocation[0] must be 0 for mapping_type A"
            assert 4 <= alloc[1] <= max_length, "symbol_allocation[1] must be in [4, 14 (or 12)]"
        else:
            assert 0 <= alloc[0] <= 13, "symbol_allocation[0] must be in [0,13] for mapping_type B"
            assert 1 <= alloc[1] <= max_length, "symbol_allocation[1] must be in [1, 14 (or 12)]"
            if dmrs.length == 2:
                assert alloc[1] >= 5, "symbol_allocation[1] must be >=5 for dmrs.length==2"
        assert alloc[0] + alloc[1] <= max_length, "symbol_allocation[0]+symbol_allocation[1] must be < 14 (or 12)"
        self._reassign(["n_size_bwp", "n_start_bwp", "num_layers", "mapping_type", "symbol_allocation", "n_rnti", "precoding",
                        "transform_precoding", "tpmi"])
        assert self.tb.channel_type == "PUSCH", 'TB_config must be configured for "PUSCH" transmission.'
        if len(dmrs.dmrs_port_set) > 0:
            assert self.num_layers == len(dmrs.dmrs_port_set), "num_layers must equal the number of DMRS ports"
        return True


def check_pusch_configs(pusch_configs):
    """validates a list of ``PUSCHConfig`` (one per transmitter) and returns the parameters ``PUSCHTransmitter`` is built
    from; those that are not per transmitter are the first configuration's"""
    assert isinstance(pusch_configs, list), "pusch_configs must be a Sequence of instances of PUSCHConfig"
    for pusch_config in pusch_configs:
        assert isinstance(pusch_config, PUSCHConfig), "All elements of pusch_configs must be instances of PUSCHConfig"
        pusch_config.check_config()
    pc = pusch_configs[0]
    params = {
        "num_bits_per_symbol": pc.tb.num_bits_per_symbol,
        "num_tx": len(pusch_configs),
        "num_layers": pc.num_layers,
        "num_subcarriers": pc.num_subcarriers,
        "num_ofdm_symbols": pc.symbol_allocation[1],
        "subcarrier_spacing": pc.carrier.subcarrier_spacing * 1e3,
        "num_antenna_ports": pc.num_antenna_ports,
        "precoding": pc.precoding,
        "precoding_matrices": [],
        "pusch_config": pc,
        "carrier_config": pc.carrier,
        "num_coded_bits": pc.num_coded_bits,
        "target_coderate": pc.tb.target_coderate,
        "n_id": [],
        "n_rnti": [],
        "tb_size": pc.tb_size,
        "dmrs_length": pc.dmrs.length,
        "dmrs_additional_position": pc.dmrs.additional_position,
        "num_cdm_groups_without_data": pc.dmrs.num_cdm_groups_without_data,
    }
    params["bandwidth"] = params["num_subcarriers"] * params["subcarrier_spacing"]
    params["cyclic_prefix_length"] = np.ceil(pc.carrier.cyclic_prefix_length * params["bandwidth"])
    for pusch_config in pusch_configs:
        if params["precoding"] == "codebook":
            params["precoding_matrices"].append(pusch_config.precoding_matrix)
        params["n_id"].append(pusch_config.carrier.n_cell_id if pusch_config.tb.n_id is None else pusch_config.tb.n_id)
        params["n_rnti"].append(pusch_config.n_rnti)
    return params
