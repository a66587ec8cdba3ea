"""Channel models for optical communications (mirror of ``sionna.phy.channel.optical``)."""
from .edfa import EDFA
from .fiber import SSFM
