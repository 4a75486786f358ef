"""redsec_amd -- MI355X-native gate-bootstrapping backend for REDsec's encrypted hot path.

Only what the path needs lives here:
  csrc/        HIP kernels (gfx950) + the C ABI declared in include/redsec_hip.h
  backend.py   ctypes binding of that ABI (torch tensors in, torch tensors out)
  arith.py     adder, subtractor and comparator on bit-sliced batches (two bootstraps per bit, on Backend.gate_rows); select,
               maximum, equal and multiply through compiled circuits
  circuit.py   netlists compiled into levelised cell tables for Backend.circuit_run (rs_circuit_run_dev)
  build.py     in-tree build of libredsec_hip.so (and the test-only lane emulator)
"""
from .backend import Backend, RedsecHipError, params, load_library, GATES, ROW_OPS, CELL_OPS, ABI_SYMBOLS  # noqa: F401

__all__ = ["Backend", "RedsecHipError", "params", "load_library", "GATES", "ROW_OPS", "CELL_OPS", "ABI_SYMBOLS"]
