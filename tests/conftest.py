import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    _load_library_first()


def _load_library_first():
    """Load libdavo_hip.so, and with it the ROCm HIP runtime it is linked against, before any test imports torch.  The torch
    wheel ships a HIP runtime of its own under the same soname (libamdhip64.so.7); once torch is imported, a library loaded
    after it binds to torch's runtime, which finds no device for it, and every GPU test after the first CPU test that
    imports torch fails.  Loading does not touch the GPU.  When the library is not built yet, test_abi.py builds and loads it
    before any torch import."""
    from davo_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        _lib.lib()


@pytest.fixture(scope="session")
def c_oracle():
    from oracle import c_oracle as C
    C.build()
    return C
