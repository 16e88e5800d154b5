import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "trex-gym_amd"))

ASSET_URDF = os.path.join(ROOT, "trex-gym_amd", "assets", "trex_collide.urdf")
# the reference project's own URDF and its 28 COLLADA hulls, stored as one archive (tests/golden/reference_assets.md)
REFERENCE_ASSETS_ARCHIVE = os.path.join(ROOT, "tests", "golden", "reference_assets.tar.xz")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


@pytest.fixture(scope="session")
def reference_assets(tmp_path_factory):
    """directory holding trex.urdf and collisions/*.dae of the reference project, unpacked from the committed archive"""
    import tarfile
    out = tmp_path_factory.mktemp("reference_assets")
    with tarfile.open(REFERENCE_ASSETS_ARCHIVE) as t:
        t.extractall(str(out), **({"filter": "data"} if hasattr(tarfile, "data_filter") else {}))
    return str(out)


@pytest.fixture(scope="session")
def model():
    from oracle import trex_model
    return trex_model.compile_model(ASSET_URDF)


@pytest.fixture(scope="session")
def oracle64(model):
    from oracle import oracle as O
    return O.Oracle(model, precision="f64")


@pytest.fixture(scope="session")
def oracle32(model):
    from oracle import oracle as O
    return O.Oracle(model, precision="f32")
