"""Generic binary linear block codes (mirror of ``sionna.phy.fec.linear``: encoders and the OSD decoder)."""
from .encoding import LinearEncoder, AllZeroEncoder
from .decoding import OSDecoder
