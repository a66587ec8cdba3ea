"""``Config`` - base of the NR configuration objects (mirror of reference src/sionna/phy/nr/config.py:10-53): keyword
arguments that name a property are set through its setter, a property reads its default the first time it is asked for."""
import copy
from abc import ABC

import numpy as np

# what show() does not print: methods, the child configurations, and arrays (their shape instead)
_NOT_SHOWN = ("show", "name", "check_config", "check_config_precoded", "clone", "c_init", "dmrs", "tb", "carrier")
_SHAPE_ONLY = ("dmrs_grid", "dmrs_grid_precoded", "dmrs_mask", "n")


class Config(ABC):
    def __init__(self, **kwargs):
        for key, value in kwargs.items():
            if key in dir(self):
                setattr(self, key, value)

    def _ifndef(self, name, value):
        if not hasattr(self, "_" + name):
            setattr(self, "_" + name, value)

    def _reassign(self, names):
        """every configurable property through its getter (default) and setter (validation) once more"""
        for name in names:
            setattr(self, name, getattr(self, name))

    def clone(self, deep=True):
        return copy.deepcopy(self) if deep else copy.copy(self)

    def check_config(self):
        pass

    def show(self):
        self.check_config()
        print(self._name)
        print("=" * len(self._name))
        for a in dir(self):
            if a.startswith("_") or a in _NOT_SHOWN:
                continue
            val = getattr(self, a)
            print(f"{a} : shape {np.array(val).shape}" if a in _SHAPE_ONLY else f"{a} : {val}")
        print("\r")
