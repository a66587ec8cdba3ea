"""``PUSCHLSChannelEstimator`` - least-squares channel estimation on the DMRS of NR PUSCH slots (mirror of reference
src/sionna/phy/nr/pusch_channel_estimation.py:9-169).  Two ports of one CDM group share their pilot resource elements, so the
plain estimates y / pilot are de-spread: averaged over the two adjacent DMRS symbols (``dmrs_length`` 2) and summed over runs
of ``2 * num_cdm_groups_without_data`` consecutive pilots of a DMRS symbol.  The reference does that behind a gather of the
pilot resource elements with a divide, two splits, two sums, two repeats, a where and three reshapes; here ONE launch,
``samd_pusch_ls_c64`` (``_c128`` with ``precision="double"``, csrc/pusch_rx.hip), goes from the received grid to the
de-spread estimates - at the pilots for the linear interpolators, or through the nearest-neighbour table over the whole
grid, which makes ``interpolation_type="nn"`` one launch in total."""
import numpy as np
import torch

from ... import _ffi
from ..block import wrap
from ..ofdm.channel_estimation import LSChannelEstimator, LinearInterpolator, NearestNeighborInterpolator


class PUSCHLSChannelEstimator(LSChannelEstimator):
    """``PUSCHLSChannelEstimator(resource_grid, dmrs_length, dmrs_additional_position, num_cdm_groups_without_data,
    interpolation_type="nn", interpolator=None)(y, no) -> (h_hat, err_var)``; y [batch, num_rx, num_rx_ant, num_ofdm_symbols,
    fft_size]; h_hat [batch, num_rx, num_rx_ant, num_tx, num_streams_per_tx, num_ofdm_symbols, num_effective_subcarriers];
    err_var broadcastable to it.  ``h_hat`` is always materialised: the deferred recipe of the base class assumes one source
    per resource element."""

    def __init__(self, resource_grid, dmrs_length, dmrs_additional_position, num_cdm_groups_without_data,
                 interpolation_type="nn", interpolator=None, precision=None, **kwargs):
        super().__init__(resource_grid, interpolation_type, interpolator, precision=precision, **kwargs)
        assert dmrs_length in (1, 2), "dmrs_length must be 1 or 2"
        assert num_cdm_groups_without_data in (1, 2, 3), "num_cdm_groups_without_data must be 1, 2 or 3"
        self._dmrs_length = int(dmrs_length)
        self._dmrs_additional_position = int(dmrs_additional_position)
        self._num_cdm_groups_without_data = int(num_cdm_groups_without_data)
        self._num_dmrs_syms = self._dmrs_length * (self._dmrs_additional_position + 1)        # :94-96
        pp = resource_grid.pilot_pattern
        self._pilot_pattern = pp
        num_pilots = int(np.asarray(pp.pilots).shape[-1])
        self._num_pilots_per_dmrs_sym = num_pilots // self._num_dmrs_syms                      # :98-101
        self._run = 2 * self._num_cdm_groups_without_data
        assert self._num_pilots_per_dmrs_sym * self._num_dmrs_syms == num_pilots and self._num_pilots_per_dmrs_sym % self._run == 0, \
            "the pilot pattern does not consist of num_dmrs_syms DMRS symbols of whole runs of 2 * num_cdm_groups_without_data pilots"
        self._defer = False
        self._tables, self._dev = None, None

    def _host_tables(self):
        """what the launch reads besides the grid, as host arrays: src [S, num_pilots] (index of the pilot's resource element
        in the full grid), coef [S, num_pilots] (1 / pilot, 0 for a zero pilot), gather [S, T * F] (number of the nearest
        pilot with energy), and the error-variance denominators den [S, num_pilots] = |pilot|^2 * 2 (* 2 with dmrs_length 2)"""
        if self._tables is None:
            rg, pp = self._rg, self._pilot_pattern
            mask = np.asarray(pp.mask)
            s = mask.shape[0] * mask.shape[1]
            pilot_re = np.stack([np.flatnonzero(m) for m in mask.reshape(s, -1)])          # row-major = pilot order
            t, f = np.divmod(pilot_re, rg.num_effective_subcarriers)
            src = (t * rg.fft_size + np.asarray(rg.effective_subcarrier_ind)[f]).astype(np.int32)
            pil = np.asarray(pp.pilots).reshape(s, -1).astype(self._np_cdtype)
            wide = pil.astype(np.complex128)
            live = wide != 0
            coef = np.where(live, 1 / np.where(live, wide, 1), 0).astype(self._np_cdtype)   # divide_no_nan as a multiply
            den = (np.abs(pil) ** 2).astype(self._np_rdtype) * self._np_rdtype(2 * self._dmrs_length)
            gather = NearestNeighborInterpolator(pp).gather_ind.reshape(s, -1).astype(np.int32)
            self._tables = {"src": src, "coef": coef, "gather": gather, "den": den, "pilots": pil}
        return self._tables

    def _device_tables(self):
        if self._dev is None:
            t = self._host_tables()
            s, num_pilots = t["src"].shape
            self._dev = {"src": _ffi.to_device(t["src"], torch.int32), "coef": _ffi.to_device(t["coef"], self.cdtype),
                         "gather": _ffi.to_device(t["gather"], torch.int32), "den": _ffi.to_device(t["den"], self.rdtype),
                         "den_nn": _ffi.to_device(np.take_along_axis(t["den"], t["gather"], axis=1), self.rdtype),
                         "identity": _ffi.to_device(np.arange(s * num_pilots, dtype=np.int32).reshape(s, num_pilots), torch.int32)}
        return self._dev

    def _launch(self, y, src, gather, rows, n_in, out, what):
        d = self._device_tables()
        s, num_pilots = d["coef"].shape
        n_out = num_pilots if gather is None else gather.shape[1]
        fn = _ffi.lib().samd_pusch_ls_c128 if self.precision == "double" else _ffi.lib().samd_pusch_ls_c64
        _ffi.check(fn(_ffi.ptr(y), _ffi.ptr(src), _ffi.ptr(d["coef"]), _ffi.ptr(gather), rows, s, num_pilots,
                      self._num_pilots_per_dmrs_sym, self._run, self._dmrs_length, n_out, n_in, _ffi.ptr(out), _ffi.stream()), what)

    @staticmethod
    def _err_var(no, den):
        """no / (|pilot|^2 * 2 [* 2]) with divide_no_nan: the reference's no / |pilot|^2 halved once or twice (:129, :148,
        :167; scaling by a power of two commutes with the rounding of the division)"""
        live = den > 0
        return torch.where(live, no / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(den))

    def estimate_at_pilot_locations(self, y_pilots, no):
        """y_pilots [batch, num_rx, num_rx_ant, num_tx, num_streams_per_tx, num_pilot_symbols] -> (h_hat of the same shape: the
        de-spread LS estimates, err_var broadcastable to it) (:103-169).  The kernel of ``call`` on the gathered pilots."""
        pp = self._pilot_pattern
        d = self._device_tables()
        s, num_pilots = d["coef"].shape
        yp = _ffi.to_device(y_pilots, self.cdtype)
        assert yp.dim() == 6 and tuple(yp.shape[3:]) == (pp.mask.shape[0], pp.mask.shape[1], num_pilots), \
            "y_pilots must have shape [batch, num_rx, num_rx_ant, num_tx, num_streams_per_tx, num_pilot_symbols]"
        rows = yp.shape[0] * yp.shape[1] * yp.shape[2]
        h_hat = torch.empty_like(yp)
        self._launch(yp, d["identity"], None, rows, s * num_pilots, h_hat, "PUSCHLSChannelEstimator.estimate_at_pilot_locations")
        no = _ffi.to_device(no, self.rdtype)
        no = no.reshape(tuple(no.shape) + (1,) * (6 - no.dim()))
        return wrap(h_hat), wrap(self._err_var(no, d["den"].reshape(tuple(pp.mask.shape[:2]) + (num_pilots,))))

    def call(self, y, no):
        rg = self._rg
        y = _ffi.to_device(y, self.cdtype)
        assert y.dim() == 5 and y.shape[-2:] == (rg.num_ofdm_symbols, rg.fft_size), \
            "y must have shape [batch, num_rx, num_rx_ant, num_ofdm_symbols, fft_size]"
        d = self._device_tables()
        nn = self._interpolation_type == "nn"
        rows = y.shape[0] * y.shape[1] * y.shape[2]
        h_hat = torch.empty(tuple(y.shape[:3]) + self._out_shape, dtype=self.cdtype, device=y.device)
        self._launch(y, d["src"], d["gather"] if nn else None, rows, rg.num_ofdm_symbols * rg.fft_size, h_hat,
                     "PUSCHLSChannelEstimator")
        # the error variance is a table of a few KB times `no` (the first n <= 3 dims of [batch, num_rx, num_rx_ant]): plain
        # broadcasting, as in LSChannelEstimator.call
        no = _ffi.to_device(no, self.rdtype)
        no = no.reshape(tuple(no.shape) + (1,) * (3 - no.dim()) + (1,) * len(self._out_shape))
        err_var = self._err_var(no, (d["den_nn"] if nn else d["den"]).reshape(self._out_shape))
        if self._lin is not None:
            # as in the base class: a foreign interpolator sees err_var broadcast to h_hat's shape (ofdm/channel_estimation.py
            # :160-163), the built-in one keeps the leading dims unexpanded
            lead = tuple(err_var.shape[:3]) if isinstance(self._lin, LinearInterpolator) else tuple(h_hat.shape[:3])
            err_var = torch.broadcast_to(err_var, lead + self._out_shape)
            h_hat, err_var = self._lin(h_hat, err_var.contiguous())
            h_hat, err_var = _ffi.to_device(h_hat, self.cdtype), _ffi.to_device(err_var, self.rdtype)
        return h_hat, torch.clamp_min(err_var, 0.)
