import os
import sys

import pytest

# Make the in-tree package importable without installation.
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real MI355X GPU (run via gpurun)"
    )


#: sockaddr_un.sun_path holds 108 bytes including the NUL, and gRPC already
#: refuses a 107-byte path; the longest socket a test binds below its
#: directory is plugins_registry/<driver>.sock.
_SUN_PATH_MAX = 104
_SOCK_SUFFIX_MAX = len("/plugins_registry/gpu.amd.com.sock")


@pytest.fixture
def sock_dir(tmp_path):
    """Directory for unix sockets. ``tmp_path`` nests under the runner's
    temp root and the test's name, which can push a socket path past the
    kernel's sun_path limit; use it when it fits, else a short directory
    of its own (removed afterwards)."""
    import pathlib
    import shutil
    import tempfile

    budget = _SUN_PATH_MAX - _SOCK_SUFFIX_MAX
    if len(os.fsencode(str(tmp_path))) <= budget:
        yield tmp_path
        return
    made = None
    for base in (tempfile.gettempdir(), "/tmp", "/dev/shm"):
        # mkdtemp appends 8 random characters to the prefix
        if len(os.fsencode(base)) + len("/dra-") + 8 > budget:
            continue
        try:
            made = tempfile.mkdtemp(prefix="dra-", dir=base)
            break
        except OSError:
            continue
    if made is None:
        pytest.fail(
            f"no writable temp directory short enough for a unix socket "
            f"(need <= {budget} bytes)"
        )
    try:
        yield pathlib.Path(made)
    finally:
        shutil.rmtree(made, ignore_errors=True)


@pytest.fixture
def fake_lib():
    from k8s_dra_driver_amd.hal import FakeDeviceLib

    lib = FakeDeviceLib()
    lib.open()
    yield lib
    lib.close()
