"""DFT-D3 dispersion (reference: nvalchemiops/interactions/dispersion/__init__.py): BJ damping, zero damping and the three-body terms."""
from nvalchemiops.interactions.dispersion.dftd3 import D3Parameters, dftd3, dftd3_atm, dftd3_zero, dftd3_zero_atm

__all__ = ["D3Parameters", "dftd3", "dftd3_atm", "dftd3_zero", "dftd3_zero_atm"]
