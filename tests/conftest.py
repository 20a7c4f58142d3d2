import atexit
import os
import shutil
import sys
import tempfile
from pathlib import Path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device)")
    config.addinivalue_line("markers", "slow: multi-process / long-running integration test")


# The tests bind Unix sockets under their temporary directory, and an AF_UNIX address holds 107
# bytes: pytest's own ``tmp_path`` (base temp / ``pytest-of-<user>`` / ``pytest-N`` / the test's
# name) can use up most of them, depending on the user's name and on where the suite is run,
# before the socket's own name.  So ``tmp_path`` here is a short directory of its own.
_SHORT_DIRS: list[str] = []


def _remove_short_dirs() -> None:
    for d in _SHORT_DIRS:
        shutil.rmtree(d, ignore_errors=True)


# registered first, so it runs last: after the exit hooks of what a test left writing there (a
# span exporter's last flush)
atexit.register(_remove_short_dirs)


def _short_tmp_dir() -> Path:
    base = tempfile.gettempdir()
    if len(base) > len("/tmp") and os.path.isdir("/tmp") and os.access("/tmp", os.W_OK | os.X_OK):
        base = "/tmp"
    d = tempfile.mkdtemp(prefix="tt-", dir=base)
    _SHORT_DIRS.append(d)
    return Path(d)


@pytest.fixture
def tmp_path():
    """A per-test directory with a short path (see above), removed when the run ends."""
    return _short_tmp_dir()


@pytest.fixture(scope="module")
def module_tmp_path():
    """``tmp_path`` for a module-scoped fixture whose directory holds an environment (its control
    socket)."""
    return _short_tmp_dir()


@pytest.fixture
def tmp_env_dir(tmp_path):
    d = tmp_path / "env"
    d.mkdir()
    return d
