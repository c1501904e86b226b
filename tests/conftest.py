import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the reference's bundled data directory (its t7 position files and *_game_counts.txt, 4401
# small files) as one archive: the ref_data fixture unpacks it once per session, so the tests
# that read the raw files need nothing outside the repository
REFERENCE_ARCHIVE = os.path.join(ROOT, "tests", "golden", "reference_data.tar.xz")
# the same data decoded by our own t7 reader and committed as packed .npz
# (tools/pack_fixture.py)
PACKED_FIXTURE = os.path.join(ROOT, "tests", "fixtures")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP kernels)")
    config.addinivalue_line("markers", "slow: long-running test")
    # an empty hipGraph capture is the symptom of a capture on the wrong device or stream:
    # SegmentedStep never produces one on purpose, so any occurrence fails the test
    config.addinivalue_line("filterwarnings", "error:The CUDA Graph is empty")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


HAS_GPU = _has_gpu()


def pytest_collection_modifyitems(config, items):
    if HAS_GPU:
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def ref_data(tmp_path_factory):
    import tarfile
    root = tmp_path_factory.mktemp("reference")
    with tarfile.open(REFERENCE_ARCHIVE) as tf:
        if hasattr(tarfile, "data_filter"):
            tf.extractall(root, filter="data")
        else:
            tf.extractall(root)
    return str(root / "data")


@pytest.fixture(scope="session")
def packed_fixture():
    return PACKED_FIXTURE
