"""Base of the signal blocks: unlike the other blocks they accept host tensors and keep them on the host, where
``convolve`` runs the specification arithmetic; arrays go to the device like everywhere else."""
import numpy as np
import torch

from ..block import Block


class SignalBlock(Block):
    def _convert_to_tensor(self, v):
        if isinstance(v, torch.Tensor):
            v = v.detach().as_subclass(torch.Tensor)
            dt = self.cdtype if v.dtype.is_complex else self.rdtype if v.dtype.is_floating_point else v.dtype
            return v if v.dtype == dt else v.to(dt)
        return super()._convert_to_tensor(v)

    def _cast_or_check_precision(self, v):
        """reference block.py:54-81: coefficients are cast to the block's real / complex dtype (kept on the host)"""
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(v))
        v = v.detach().as_subclass(torch.Tensor).cpu()
        return v.to(self.cdtype if v.dtype.is_complex else self.rdtype)
