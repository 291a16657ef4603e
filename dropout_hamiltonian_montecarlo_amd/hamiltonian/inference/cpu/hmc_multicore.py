"""hamiltonian.inference.cpu.hmc_multicore — import path of the reference's inference/cpu/hmc_multicore.py, served by
the libhmcx sampler of hamiltonian.inference.gpu.hmc_multicore (NumPy in / NumPy out, same signatures)."""
from ..gpu.hmc_multicore import hmc_multicore  # noqa: F401
