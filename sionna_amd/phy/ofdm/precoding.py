"""Precoding of OFDM resource grids - mirror of reference src/sionna/phy/ofdm/precoding.py (``RZFPrecoder`` :15-177).
The whole ``call`` (gather of the intended receivers' channels through ``StreamManagement.precoding_ind``, the RZF
precoding matrix per resource element, G x, and the effective channel H_r G of every receiver at the effective
subcarriers) is ONE HIP kernel, ``samd_rzf_precode_ofdm_c64`` / ``_c128`` (csrc/precoding.hip)."""
import numpy as np
import torch

from ... import _ffi
from ..block import Block
from ..mimo.precoding import expand_alpha, _shape


class RZFPrecoder(Block):
    """Regularised zero-forcing precoding of resource grids for every transmitter towards its intended receivers.

    ``call(x, h, alpha=0.)``: x [B, num_tx, num_streams_per_tx, T, fft_size], h [B, num_rx, num_rx_ant, num_tx, num_tx_ant,
    T, fft_size], alpha broadcastable to [B, num_tx, T, fft_size] -> x_precoded [B, num_tx, num_tx_ant, T, fft_size] and,
    with ``return_effective_channel``, h_eff [B, num_rx, num_rx_ant, num_tx, num_streams_per_tx, T,
    num_effective_subcarriers] (nulled subcarriers removed)."""

    def __init__(self, resource_grid, stream_management, return_effective_channel=False, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        from .resource_grid import ResourceGrid
        from ..mimo.stream_management import StreamManagement
        assert isinstance(resource_grid, ResourceGrid)
        assert isinstance(stream_management, StreamManagement)
        self._resource_grid, self._stream_management = resource_grid, stream_management
        self._return_effective_channel = return_effective_channel
        self._dev = None

    def _tables(self):
        """(precoding_ind [TX, num_rx_per_tx], position of every subcarrier among the effective ones or -1 [F]) on the device,
        built once per block."""
        if self._dev is None:
            rg, sm = self._resource_grid, self._stream_management
            pind = np.ascontiguousarray(sm.precoding_ind, np.int32).reshape(sm.num_tx, -1)
            if pind.size and (pind.min() < 0 or pind.max() >= sm.num_rx):
                raise ValueError("RZFPrecoder: StreamManagement.precoding_ind names a receiver that does not exist")
            eff = np.full(rg.fft_size, -1, np.int32)
            eff[np.asarray(rg.effective_subcarrier_ind, np.int64)] = np.arange(rg.num_effective_subcarriers, dtype=np.int32)
            self._dev = (_ffi.to_device(pind, torch.int32), _ffi.to_device(eff, torch.int32), pind.shape[1])
        return self._dev

    def _check(self, xs, hs):
        rg, sm = self._resource_grid, self._stream_management
        want_x = (rg.num_tx, rg.num_streams_per_tx, rg.num_ofdm_symbols, rg.fft_size)
        if len(xs) != 5 or tuple(xs[1:]) != want_x:
            raise ValueError(f"RZFPrecoder: x must have shape [batch_size, {', '.join(map(str, want_x))}], got {xs}")
        if len(hs) != 7 or hs[0] != xs[0] or hs[1] != sm.num_rx or hs[3] != rg.num_tx or \
                tuple(hs[5:]) != (rg.num_ofdm_symbols, rg.fft_size):
            raise ValueError(f"RZFPrecoder: h must have shape [{xs[0] if xs else 'batch_size'}, {sm.num_rx}, num_rx_ant, "
                             f"{rg.num_tx}, num_tx_ant, {rg.num_ofdm_symbols}, {rg.fft_size}], got {hs}")
        if sm.num_tx != rg.num_tx or sm.num_streams_per_tx != rg.num_streams_per_tx:
            raise ValueError("RZFPrecoder: the ResourceGrid and the StreamManagement disagree on the transmitters or streams")
        nrxt = np.asarray(sm.precoding_ind).reshape(sm.num_tx, -1).shape[1]
        k, m = nrxt * int(hs[2]), int(hs[4])
        if k != rg.num_streams_per_tx:
            raise ValueError(f"RZFPrecoder: {nrxt} intended receivers x {hs[2]} antennas = {k} channel rows, but "
                             f"{rg.num_streams_per_tx} streams per transmitter")
        if k > m:
            raise ValueError(f"RZFPrecoder: K = {k} streams exceed M = {m} transmit antennas (K <= M required)")
        if k > 16 or m > 32:
            raise ValueError(f"RZFPrecoder: supported up to K = 16 streams and M = 32 transmit antennas (got K = {k}, M = {m})")

    def __call__(self, x, h, alpha=0., **kwargs):
        self._check(_shape(x), _shape(h))                 # before Block.__call__ moves the arguments to the device
        return super().__call__(x, h, alpha, **kwargs)

    def call(self, x, h, alpha=0.):
        rg = self._resource_grid
        xs, hs = _shape(x), _shape(h)
        self._check(xs, hs)
        dbl = self.precision == "double"
        cdt, rdt = (torch.complex128, torch.float64) if dbl else (torch.complex64, torch.float32)
        x = _ffi.to_device(x, cdt)
        h = _ffi.to_device(h, cdt)
        b, ntx, ns, t, f = xs
        rx, rxa, mtx = hs[1], hs[2], hs[4]
        a0, a = expand_alpha(alpha, (b, ntx, t, f), rdt, leading_axis=True)
        pind, eff, nrxt = self._tables()
        fe = rg.num_effective_subcarriers
        xp = torch.empty((b, ntx, mtx, t, f), dtype=cdt, device=x.device)
        he = torch.empty((b, rx, rxa, ntx, ns, t, fe), dtype=cdt, device=x.device) if self._return_effective_channel else None
        fn = _ffi.lib().samd_rzf_precode_ofdm_c128 if dbl else _ffi.lib().samd_rzf_precode_ofdm_c64
        _ffi.check(fn(_ffi.ptr(x), _ffi.ptr(h), _ffi.ptr(a), a0, _ffi.ptr(pind), _ffi.ptr(eff), b, ntx, ns, rx, rxa, mtx, nrxt,
                      t, f, fe, _ffi.ptr(xp), _ffi.ptr(he), _ffi.stream()), "RZFPrecoder")
        return (xp, he) if self._return_effective_channel else xp
