"""The `warmstart` model parameter (PGS warm start of the contact rows): host side only, no GPU needed."""
import math

import pytest

from conftest import ASSET_URDF


@pytest.fixture
def model():
    from trex_gym import _capi
    return _capi.Model(ASSET_URDF)


def test_warmstart_defaults_to_off(model):
    assert model.get_param("warmstart") == 0.0


@pytest.mark.parametrize("value", [0.0, 0.5, 0.85, 1.0])
def test_warmstart_round_trips(model, value):
    model.set_param("warmstart", value)
    assert model.get_param("warmstart") == value


@pytest.mark.parametrize("value", [-0.1, 1.5, math.nan, math.inf])
def test_warmstart_out_of_range_is_refused(model, value):
    from trex_gym import _capi
    model.set_param("warmstart", 0.85)
    with pytest.raises(_capi.TrexError):
        model.set_param("warmstart", value)
    assert model.get_param("warmstart") == 0.85       # a refused value changes nothing


def test_unknown_parameter_names_are_still_refused(model):
    from trex_gym import _capi
    for name in ("warm_start", "Warmstart", "warmstart_factor"):
        with pytest.raises(_capi.TrexError):
            model.set_param(name, 0.5)
        with pytest.raises(_capi.TrexError):
            model.get_param(name)


def test_trainer_forwards_warmstart():
    import inspect
    from trex_gym import trex_train
    assert "warmstart" in inspect.signature(trex_train.build_environment).parameters
