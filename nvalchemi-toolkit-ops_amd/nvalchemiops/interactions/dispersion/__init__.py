"""DFT-D3(BJ) dispersion (reference: nvalchemiops/interactions/dispersion/__init__.py) and its three-body term."""
from nvalchemiops.interactions.dispersion.dftd3 import D3Parameters, dftd3, dftd3_atm

__all__ = ["D3Parameters", "dftd3", "dftd3_atm"]
