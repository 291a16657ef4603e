"""hamiltonian.inference.cpu.metropolis — import path of the reference's inference/cpu/metropolis.py, served by
the libhmcx sampler of hamiltonian.inference.gpu.metropolis (NumPy in / NumPy out, same signatures)."""
from ..gpu.metropolis import MH  # noqa: F401
