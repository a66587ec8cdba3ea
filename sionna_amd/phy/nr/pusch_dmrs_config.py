"""``PUSCHDMRSConfig`` - demodulation reference signals of a PUSCH, 38.211 Sec. 6.4.1.1 (mirror of reference
src/sionna/phy/nr/pusch_dmrs_config.py:11-351).  The per-port parameters are Tables 6.4.1.1.3-1 (configuration type 1,
ports 0..7) and 6.4.1.1.3-2 (type 2, ports 0..11)."""
from collections.abc import Sequence

import numpy as np

from .config import Config

# per DMRS port: CDM group, frequency shift Delta, sign of w_f(1), sign of w_t(1)
_PORTS = {1: {"cdm": [0, 0, 1, 1] * 2, "delta": [0, 0, 1, 1] * 2, "wf1": [1, -1] * 4, "wt1": [1] * 4 + [-1] * 4},
          2: {"cdm": [0, 0, 1, 1, 2, 2] * 2, "delta": [0, 0, 2, 2, 4, 4] * 2, "wf1": [1, -1] * 6, "wt1": [1] * 6 + [-1] * 6}}


class PUSCHDMRSConfig(Config):
    def __init__(self, **kwargs):
        self._name = "PUSCH DMRS Configuration"
        super().__init__(**kwargs)
        self.check_config()

    # ---- configurable
    @property
    def config_type(self):
        self._ifndef("config_type", 1)
        return self._config_type

    @config_type.setter
    def config_type(self, value):
        assert value in [1, 2], "config_type must be in [1,2]"
        self._config_type = value

    @property
    def type_a_position(self):
        self._ifndef("type_a_position", 2)
        return self._type_a_position

    @type_a_position.setter
    def type_a_position(self, value):
        assert value in [2, 3], "type_a_position must be in [2,3]"
        self._type_a_position = value

    @property
    def additional_position(self):
        self._ifndef("additional_position", 0)
        return self._additional_position

    @additional_position.setter
    def additional_position(self, value):
        assert value in [0, 1, 2, 3], "additional_position must be in [0,1,2,3]"
        self._additional_position = value

    @property
    def length(self):
        self._ifndef("length", 1)
        return self._length

    @length.setter
    def length(self, value):
        assert value in [1, 2], "Invalid DMRS length"
        self._length = value

    @property
    def dmrs_port_set(self):
        self._ifndef("dmrs_port_set", [])
        return self._dmrs_port_set

    @dmrs_port_set.setter
    def dmrs_port_set(self, value):
        if isinstance(value, int):
            value = [value]
        elif isinstance(value, Sequence):
            value = list(value)
        else:
            raise ValueError("dmrs_port_set must be an integer or list")
        self._dmrs_port_set = value

    @property
    def n_id(self):
        self._ifndef("n_id", None)
        return self._n_id

    @n_id.setter
    def n_id(self, value):
        if value is None:
            self._n_id = None
        elif isinstance(value, int):
            assert value in range(65536), "n_id must be in [0, 65535]"
            self._n_id = [value, value]
        else:
            assert len(value) == 2, "n_id must be either [] or a two-tuple"
            for e in value:
                assert e in range(65536), "Each element of n_id must be in [0, 65535]"
            self._n_id = value

    @property
    def n_scid(self):
        self._ifndef("n_scid", 0)
        return self._n_scid

    @n_scid.setter
    def n_scid(self, value):
        assert value in [0, 1], "n_scid must be 0 or 1"
        self._n_scid = value

    @property
    def num_cdm_groups_without_data(self):
        self._ifndef("num_cdm_groups_without_data", 2)
        return self._num_cdm_groups_without_data

    @num_cdm_groups_without_data.setter
    def num_cdm_groups_without_data(self, value):
        assert value in [1, 2, 3], "num_cdm_groups_without_data must be in [1,2,3]"
        self._num_cdm_groups_without_data = value

    # ---- read-only
    @property
    def allowed_dmrs_ports(self):
        """the ports of the CDM groups without data: two per group, and with double-symbol DMRS their time-domain twins"""
        groups = min(self.num_cdm_groups_without_data, 2 if self.config_type == 1 else 3)
        first = list(range(2 * groups))
        if self.length == 1:
            return first
        return first + [p + (4 if self.config_type == 1 else 6) for p in first]

    def _per_port(self, key):
        row = _PORTS[self.config_type][key]
        return [row[port] for port in self.dmrs_port_set]

    @property
    def cdm_groups(self):
        return self._per_port("cdm")

    @property
    def deltas(self):
        return self._per_port("delta")

    @property
    def w_f(self):
        """[2, num_ports]: w_f(k') for k' = 0, 1"""
        row = np.array(_PORTS[self.config_type]["wf1"])
        return np.stack([np.ones_like(row), row])[:, self.dmrs_port_set]

    @property
    def w_t(self):
        """[2, num_ports]: w_t(l') for l' = 0, 1"""
        row = np.array(_PORTS[self.config_type]["wt1"])
        return np.stack([np.ones_like(row), row])[:, self.dmrs_port_set]

    @property
    def beta(self):
        """ratio of PUSCH to DMRS energy per resource element, 38.214 Table 6.2.2-1 (three groups: type 2 only)"""
        n = self.num_cdm_groups_without_data
        if n == 1:
            return 1.0
        if n == 2:
            return np.sqrt(2)
        return np.sqrt(3) if self.config_type == 2 else None

    def check_config(self):
        if self.length == 2:
            assert self.additional_position in [0, 1], "additional_position must be in [0, 1] for length==2"
        for p in self.dmrs_port_set:
            assert p in self.allowed_dmrs_ports, f"Unallowed DMRS port {p}. Not in {self.allowed_dmrs_ports}."
        if self.config_type == 1:
            assert self.num_cdm_groups_without_data in [1, 2], "num_cdm_groups_without_data must be in [1,2] for config_type 1"
        self._reassign(["config_type", "type_a_position", "additional_position", "length", "dmrs_port_set", "n_id", "n_scid",
                        "num_cdm_groups_without_data"])
