"""Physical constants the blocks of this package use, under the names ``sionna.phy.constants`` gives them."""

H = 6.62607015e-34   # Planck constant in J/Hz (exact by the 2019 SI definition): ASE noise densities of SSFM and EDFA
