"""Build the library, load it, ask for a GPU: one function, and the module fixtures on top of it (imported by name where they are used)."""
import types

import pytest


def namespace(gpu="assert"):
    """torch and the product's layers behind short names, the library built and loaded.  gpu: 'assert' a visible GPU, 'skip' the
    caller without one, or None (host tests: nothing is launched)"""
    import torch
    import ssa_gym_amd
    from ssa_gym_amd import _lib, device, engine, host
    ssa_gym_amd.build()
    _lib.load()
    if gpu == "assert":
        assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    elif gpu == "skip" and not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return types.SimpleNamespace(torch=torch, lib=_lib, dev=device, host=host, engine=engine, pkg=ssa_gym_amd)


@pytest.fixture(scope="module")
def hip():
    return namespace()


@pytest.fixture(scope="module")
def envs():
    namespace("skip")
    from ssa_gym_amd import envs as E
    return E


@pytest.fixture(scope="module")
def dev():
    return namespace("skip").dev


@pytest.fixture(scope="module")
def lib():
    """the loaded library itself (host tests: no GPU asked for)"""
    return namespace(None).lib.load()


@pytest.fixture(scope="module")
def pkg():
    return namespace(None).pkg
