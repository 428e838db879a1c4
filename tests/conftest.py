import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _raise_fd_limit(n: int = 16384):
    """One ephemeral ledger holds ~100 descriptors (11 SQLite files x database + WAL + shm x the Python
    connection and the writer's materialisers) until the collector finalises it, and many tests keep two or
    more: an ordinary user's soft limit of 1,024 does not hold a session. Raise it as far as the hard limit
    allows, as the node does at start (utils/cpus.py presize_fd_table); child processes inherit it."""
    import resource
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = n if hard == resource.RLIM_INFINITY else min(n, hard)
    if soft != resource.RLIM_INFINITY and soft < want:
        resource.setrlimit(resource.RLIMIT_NOFILE, (want, hard))


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (HIP device)')
    config.addinivalue_line('markers', 'slow: long-running test')
    _raise_fd_limit()
    # build the in-tree extension once per session (cached; no-op when up to date)
    from upow_amd import _build
    _build.build(verbose=False)


@pytest.fixture(scope='session')
def native():
    from upow_amd.ops.native import lib
    return lib()


@pytest.fixture(scope='session')
def gpu(native):
    from upow_amd.ops.native import gpu_available
    if not gpu_available():
        pytest.fail('gpu-marked test ran without a visible HIP device')
    import torch
    torch.cuda.set_device(0)
    return native
