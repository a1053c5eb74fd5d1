"""TEST INFRASTRUCTURE ONLY -- the pytest fixtures the host test modules share.  At module level of a test module:

    from hostsim.fixtures import built, npm_fixture
    npm = npm_fixture('paged')
"""

import os

import pytest

from . import install, uninstall


def activate(profile=None):
    """``install(profile)`` for a test: the package, its simulator as ``.sim``, no communicator left over."""
    import np_modeling_amd
    from np_modeling_amd import parallel
    np_modeling_amd.sim = install(profile)
    parallel.set_communicator(None)
    return np_modeling_amd


def deactivate():
    from np_modeling_amd import parallel
    parallel.set_communicator(None)
    uninstall()


def npm_fixture(profile=None):
    """``npm = npm_fixture('paged')`` at module level: the fixture ``npm`` of that module."""
    @pytest.fixture
    def npm():
        package = activate(profile)
        sim = package.sim                 # its memory outlives a test that installs another simulator over it  # noqa: F841
        yield package
        deactivate()
    return npm


@pytest.fixture(scope='module')
def built():
    """The real library, built on the CPU where it is not there yet: ``from hostsim.fixtures import built``."""
    import __graft_entry__ as entry
    from np_modeling_amd import _C
    if not (os.path.exists(_C.LIB_PATH) and os.path.exists(_C.RCCL_LIB_PATH)):
        entry.build()
    return _C
