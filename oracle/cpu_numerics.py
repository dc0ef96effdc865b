"""Fixed CPU arithmetic for the golden fixtures.  TEST INFRASTRUCTURE.

tests/golden/ holds the reference's fp32 outputs, and the tests require the oracle to reproduce several of them bit for bit.
That holds only when the fixture was recorded with the same CPU code paths the test runs: by default MKL picks its kernels by
CPU vendor and instruction set, oneDNN JIT-compiles its convolutions for the host, ATen vectorises for the widest ISA it finds,
and reductions split their work by thread count.  Importing this module pins all four to choices every x86-64 host makes
alike -- for oracle/gen_golden*.py (through ref_harness) when it records the fixtures and for tests/conftest.py when they are
checked.  MKL and ATen read these variables at their first call, so the module must be imported before any CPU arithmetic."""
import os

os.environ["MKL_CBWR"] = "COMPATIBLE"            # MKL's vendor-independent code path
os.environ["ATEN_CPU_CAPABILITY"] = "default"    # ATen's non-vectorised kernels

import torch  # noqa: E402

THREADS = 8

torch.backends.mkldnn.enabled = False            # convolutions through ATen + MKL instead of host-tuned oneDNN kernels
torch.set_num_threads(THREADS)
assert torch.backends.cpu.get_cpu_capability() == "DEFAULT", "oracle.cpu_numerics was imported after ATen chose its kernels"
