import os
import sys

import pytest

# torch's own HIP runtime goes into the process before anything loads libeazy_amd.so: the library
# binds to the copy already loaded, while loaded first (test_capi, in a whole-suite run) it brings
# the system's copy, torch then loads a second runtime, and torch.cuda.is_available() is False for
# every GPU test after it
import torch  # noqa: F401,E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs on the GPU box)")


@pytest.fixture(scope="session")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")
