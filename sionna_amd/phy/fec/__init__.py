"""Forward error correction blocks of the hot path (LDPC 5G, Polar 5G, convolutional and turbo codes, CRC, scrambling,
interleaving, generic linear encoder, code utilities)."""
from . import ldpc
from . import polar, crc, scrambling, interleaving, linear, utils, conv, turbo
