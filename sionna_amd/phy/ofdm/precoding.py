"""Precoding of OFDM resource grids - mirror of reference src/sionna/phy/ofdm/precoding.py (``RZFPrecoder`` :15-177,
``PrecodedChannel`` and its RZF / CBF / identity forms :179-566).
The whole ``call`` of ``RZFPrecoder`` (gather of the intended receivers' channels through
``StreamManagement.precoding_ind``, the RZF precoding matrix per resource element, G x, and the effective channel H_r G of
every receiver at the effective subcarriers) is ONE HIP kernel, ``samd_rzf_precode_ofdm_c64`` / ``_c128``; the whole
``call`` of a precoded channel (gather from the channel knowledge, G, the transmit powers, H_r G from the true channel) is
ONE launch of ``samd_precoded_channel_c64`` / ``_c128`` (both csrc/precoding.hip)."""
from abc import abstractmethod

import numpy as np
import torch

from ... import _ffi
from ..block import Block
from ..mimo.precoding import MODE_RZF, MODE_CBF, expand_alpha, _shape

MODE_EYE = 2                                # SAMD_PRECODE_EYE (include/sionna_amd.h)


def _item(v):
    """a 0-d host array as a Python number (Block.__call__ would move it to the device as a 1-element tensor)"""
    return v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v


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


class PrecodedChannel(Block):
    """Abstract base class of the effective channel after precoding (ofdm/precoding.py:179-373):
    H~_ij = H_ij G_j diag(sqrt(p_j1), ..., sqrt(p_jS)).

    ``call(h, tx_power, h_hat=None, ...)``: h, h_hat [B, num_rx, num_rx_ant, num_tx, num_tx_ant, T, fft_size], tx_power
    [B, num_tx, num_streams_per_tx, T, fft_size] or its first n dims -> h_eff [B, num_rx, num_rx_ant, num_tx,
    num_streams_per_tx, T, num_effective_subcarriers].  The precoder is computed from ``h_hat`` (``h`` when None), the
    effective channel from the true ``h``.

    The subclasses of this package run one fused launch.  ``get_desired_channels``, ``compute_effective_channel`` and
    ``apply_tx_power`` are the reference's public helpers as plain device tensor operations (not the hot path): a
    subclass with another precoder composes its ``call`` from them as the reference's subclasses do."""

    _MODE = None

    def __init__(self, resource_grid, stream_management, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        from .resource_grid import ResourceGrid, RemoveNulledSubcarriers
        from ..mimo.stream_management import StreamManagement
        assert isinstance(resource_grid, ResourceGrid)
        assert isinstance(stream_management, StreamManagement)
        self._resource_grid, self._stream_management = resource_grid, stream_management
        self._remove_nulled_scs = RemoveNulledSubcarriers(resource_grid, precision=self.precision)
        self._dev = None

    # ---- the reference's helpers (torch) ----
    def get_desired_channels(self, h_hat):
        """h_hat [B, rx, rxa, tx, M, T, F] -> h_pc_desired [B, tx, T, F, num_streams_per_tx, M] (:246-295)"""
        sm = self._stream_management
        h_hat = _ffi.to_device(h_hat, self.cdtype)
        pind = torch.as_tensor(np.asarray(sm.precoding_ind, np.int64).reshape(sm.num_tx, -1), device=h_hat.device)
        hp = h_hat.permute(3, 1, 2, 4, 5, 6, 0)                                     # [tx, rx, rxa, M, T, F, B]
        hp = torch.stack([hp[j].index_select(0, pind[j]) for j in range(sm.num_tx)])  # [tx, rx_per_tx, rxa, M, T, F, B]
        hp = hp.reshape((hp.shape[0], hp.shape[1] * hp.shape[2]) + tuple(hp.shape[3:]))
        hp = hp.permute(5, 0, 3, 4, 1, 2)
        if hp.shape[-2] != sm.num_streams_per_tx:
            raise ValueError("The required number of streams per transmitter does not match the channel dimensions")
        return hp

    def compute_effective_channel(self, h, g):
        """h [B, rx, rxa, tx, M, T, F], g [B, tx, T, F, M, K] -> h_eff [B, rx, rxa, tx, K, T, Fe] (:297-346)"""
        g = _ffi.to_device(g, self.cdtype)
        h = _ffi.to_device(h, self.cdtype).permute(0, 1, 3, 5, 6, 2, 4)             # [B, rx, tx, T, F, rxa, M]
        h_eff = torch.matmul(h, g.unsqueeze(1)).permute(0, 1, 5, 2, 6, 3, 4)
        return self._remove_nulled_scs(h_eff.contiguous())

    def apply_tx_power(self, g, tx_power):
        """g [B, tx, T, F, M, K], tx_power [B, tx, K, T, F] or its first n dims -> g diag(sqrt(tx_power)) (:348-369)"""
        g = _ffi.to_device(g, self.cdtype)
        p = _ffi.to_device(tx_power, self.rdtype)
        p = p.reshape(tuple(p.shape) + (1,) * (6 - p.dim())).permute(0, 1, 3, 4, 5, 2)
        return torch.sqrt(torch.broadcast_to(p, g.shape)).to(self.cdtype) * g

    # ---- the fused launch ----
    def _tables(self):
        """(precoding_ind [TX, num_rx_per_tx], position of every subcarrier among the effective ones or -1 [F]) on the device"""
        if self._dev is None:
            rg, sm = self._resource_grid, self._stream_management
            pind = np.ascontiguousarray(sm.precoding_ind, np.int32).reshape(sm.num_tx, -1)
            if pind.size and (pind.min() < 0 or pind.max() >= sm.num_rx):
                raise ValueError(f"{type(self).__name__}: StreamManagement.precoding_ind names a receiver that does not exist")
            eff = np.full(rg.fft_size, -1, np.int32)
            eff[np.asarray(rg.effective_subcarrier_ind, np.int64)] = np.arange(rg.num_effective_subcarriers, dtype=np.int32)
            self._dev = (_ffi.to_device(pind, torch.int32), _ffi.to_device(eff, torch.int32), pind.shape[1])
        return self._dev

    def _check(self, hs, ps, hhs=None, als=None):
        """shapes of h, tx_power, h_hat and alpha; raises before anything moves to the device"""
        rg, sm, name = self._resource_grid, self._stream_management, type(self).__name__
        if sm.num_tx != rg.num_tx or sm.num_streams_per_tx != rg.num_streams_per_tx:
            raise ValueError(f"{name}: the ResourceGrid and the StreamManagement disagree on the transmitters or streams")
        if len(hs) != 7 or hs[1] != sm.num_rx or hs[3] != rg.num_tx or tuple(hs[5:]) != (rg.num_ofdm_symbols, rg.fft_size):
            raise ValueError(f"{name}: h must have shape [batch_size, {sm.num_rx}, num_rx_ant, {rg.num_tx}, num_tx_ant, "
                             f"{rg.num_ofdm_symbols}, {rg.fft_size}], got {hs}")
        if hhs is not None and tuple(hhs) != tuple(hs):
            raise ValueError(f"{name}: h_hat must have the shape of h {hs}, got {hhs}")
        k, m = rg.num_streams_per_tx, int(hs[4])
        if self._MODE == MODE_EYE:
            if k != m:
                raise ValueError(f"{name}: the identity precoder needs num_streams_per_tx = num_tx_ant (K == M), got "
                                 f"K = {k}, M = {m}")
        else:
            nrxt = np.asarray(sm.precoding_ind).reshape(sm.num_tx, -1).shape[1]
            if nrxt * int(hs[2]) != k:
                raise ValueError(f"{name}: {nrxt} intended receivers x {hs[2]} antennas = {nrxt * int(hs[2])} channel rows, "
                                 f"but {k} streams per transmitter")
            if k > m:
                raise ValueError(f"{name}: K = {k} streams exceed M = {m} transmit antennas (K <= M required)")
        if k > 16 or m > 32:
            raise ValueError(f"{name}: supported up to K = 16 streams and M = 32 transmit antennas (got K = {k}, M = {m})")
        full = (hs[0], rg.num_tx, k, rg.num_ofdm_symbols, rg.fft_size)
        if len(ps) > 5 or tuple(ps) != full[:len(ps)]:
            raise ValueError(f"{name}: tx_power must have shape {list(full)} or its first n dims, got {ps}")
        full = (hs[0], rg.num_tx, rg.num_ofdm_symbols, rg.fft_size)
        if als is not None and (len(als) > 4 or tuple(als) != full[:len(als)]):
            raise ValueError(f"{name}: alpha must have shape {list(full)} or its first n dims, got {als}")

    def _fused(self, h, tx_power, h_hat=None, alpha=0.):
        rg = self._resource_grid
        hs = _shape(h)
        self._check(hs, _shape(tx_power), None if h_hat is None else _shape(h_hat),
                    _shape(alpha) if self._MODE == MODE_RZF else None)
        dbl = self.precision == "double"
        cdt, rdt = (torch.complex128, torch.float64) if dbl else (torch.complex64, torch.float32)
        h = _ffi.to_device(h, cdt)
        h_hat = h if h_hat is None else _ffi.to_device(h_hat, cdt)
        b, rx, rxa, ntx, mtx, t, f = hs
        k, fe = rg.num_streams_per_tx, rg.num_effective_subcarriers
        a0, a = expand_alpha(alpha, (b, ntx, t, f), rdt) if self._MODE == MODE_RZF else (0.0, None)
        p0, p = expand_alpha(tx_power, (b, ntx, k, t, f), rdt)
        pind, eff, nrxt = self._tables()
        he = torch.empty((b, rx, rxa, ntx, k, t, fe), dtype=cdt, device=h.device)
        fn = _ffi.lib().samd_precoded_channel_c128 if dbl else _ffi.lib().samd_precoded_channel_c64
        _ffi.check(fn(_ffi.ptr(h), _ffi.ptr(h_hat), _ffi.ptr(a), a0, _ffi.ptr(p), p0, _ffi.ptr(pind), _ffi.ptr(eff), self._MODE,
                      b, ntx, k, rx, rxa, mtx, nrxt, t, f, fe, _ffi.ptr(he), _ffi.stream()), type(self).__name__)
        return he

    @abstractmethod
    def call(self, h, tx_power, h_hat=None, **kwargs):
        pass


class RZFPrecodedChannel(PrecodedChannel):
    """Effective channel after regularised zero-forcing precoding (ofdm/precoding.py:375-446), one fused launch.

    ``call(h, tx_power, h_hat=None, alpha=0.)``; alpha [B, num_tx, T, fft_size] or its first n dims (the reference expands
    it with trailing unit dimensions here, :432, unlike ``RZFPrecoder``); K <= M, K <= 16, M <= 32."""

    _MODE = MODE_RZF

    def __call__(self, h, tx_power, h_hat=None, alpha=0., **kwargs):
        self._check(_shape(h), _shape(tx_power), None if h_hat is None else _shape(h_hat), _shape(alpha))
        return super().__call__(h, _item(tx_power), h_hat=h_hat, alpha=_item(alpha), **kwargs)

    def call(self, h, tx_power, h_hat=None, alpha=0.):
        return self._fused(h, tx_power, h_hat, alpha)


class CBFPrecodedChannel(PrecodedChannel):
    """Effective channel after conjugate beamforming (ofdm/precoding.py:448-510), one fused launch.
    ``call(h, tx_power, h_hat=None)``; K <= M, K <= 16, M <= 32."""

    _MODE = MODE_CBF

    def __call__(self, h, tx_power, h_hat=None, **kwargs):
        self._check(_shape(h), _shape(tx_power), None if h_hat is None else _shape(h_hat))
        return super().__call__(h, _item(tx_power), h_hat=h_hat, **kwargs)

    def call(self, h, tx_power, h_hat=None):
        return self._fused(h, tx_power, h_hat)


class EyePrecodedChannel(PrecodedChannel):
    """Effective channel after power allocation without precoding - the identity precoder (ofdm/precoding.py:513-566), one
    fused launch.  ``call(h, tx_power)``; needs num_streams_per_tx = num_tx_ant (ValueError otherwise), at most 16."""

    _MODE = MODE_EYE

    def __call__(self, h, tx_power, **kwargs):
        self._check(_shape(h), _shape(tx_power))
        return super().__call__(h, _item(tx_power), **kwargs)

    def call(self, h, tx_power):
        return self._fused(h, tx_power)
