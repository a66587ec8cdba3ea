"""``TBConfig`` - transport-block parameters chosen by MCS table and index, 38.214 Sec. 5.1.3.1 / 6.1.4.1 (mirror of
reference src/sionna/phy/nr/tb_config.py:9-409)."""
from .config import Config
from .utils import decode_mcs_index


class TBConfig(Config):
    def __init__(self, **kwargs):
        self._name = "Transport Block Configuration"
        super().__init__(**kwargs)
        self.check_config()

    # ---- configurable
    @property
    def mcs_index(self):
        self._ifndef("mcs_index", 14)                     # 16-QAM, rate 0.54
        return self._mcs_index

    @mcs_index.setter
    def mcs_index(self, value):
        assert value in range(29), "mcs_index must be in range from 0 to 28."
        self._mcs_index = value

    @property
    def mcs_table(self):
        self._ifndef("mcs_table", 1)
        return self._mcs_table

    @mcs_table.setter
    def mcs_table(self, value):
        assert value in range(1, 5), "mcs_table must be in range from 1 to 4"
        self._mcs_table = value

    @property
    def channel_type(self):
        self._ifndef("channel_type", "PUSCH")
        return self._channel_type

    @channel_type.setter
    def channel_type(self, value):
        assert value in ("PUSCH", "PDSCH"), 'Only "PUSCH" and "PDSCH are supported'
        self._channel_type = value

    @property
    def n_id(self):
        self._ifndef("n_id", None)
        return self._n_id

    @n_id.setter
    def n_id(self, value):
        if value is not None:
            assert value in range(1024), "n_id must be in range from 0 to 1023"
        self._n_id = value

    # ---- read-only
    @property
    def name(self):
        return "Transport Block Configuration"

    def _mcs(self):
        return decode_mcs_index(self._mcs_index, self._mcs_table, is_pusch=self._channel_type == "PUSCH")

    @property
    def target_coderate(self):
        return self._mcs()[1]

    @property
    def num_bits_per_symbol(self):
        return self._mcs()[0]

    @property
    def tb_scaling(self):
        return 1.                                         # 38.214 Table 5.1.3.2-2: only 1 is supported

    def check_config(self):
        self._reassign(["mcs_index", "mcs_table", "channel_type", "n_id"])
