"""Dynamics randomisation (include/dronenav.h dn_enable_dynamics) without a GPU: the C struct against its ctypes twin, the exported
symbols, and the host-side validation of DynamicsRandomization."""

import pytest

import abi_support as abi

NEW_SYMBOLS = ("dn_enable_dynamics", "dn_set_dynamics", "dn_get_dynamics", "dn_get_dynamics_config")


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    return p


def test_dynamics_config_layout_matches_header(pkg):
    abi.check_layout(pkg._capi.DnDynamicsConfig, 40)
    abi.check_version()


def test_dynamics_symbols_are_exported_and_bound(pkg):
    abi.check_names(*NEW_SYMBOLS)


@pytest.mark.parametrize("bad", [dict(mass=(1.2, 0.8)), dict(inertia=(0.0, 1.0)), dict(kf=(-0.5, 1.0)), dict(km=(float("nan"), 1.0)),
                                 dict(mass=(1.0, float("nan"))), dict(kf=(1.0, float("inf"))), dict(inertia=(float("-inf"), 1.0)),
                                 dict(km=(1.0,))])
def test_dynamics_randomization_rejects_bad_ranges(pkg, bad):
    with pytest.raises(ValueError):
        pkg.DynamicsRandomization(**bad)


def test_dynamics_randomization_defaults_and_c_image(pkg):
    d = pkg.DynamicsRandomization()
    assert (d.mass, d.inertia, d.kf, d.km, d.resample) == ((1.0, 1.0),) * 4 + (True,)
    c = pkg.DynamicsRandomization(mass=(0.8, 1.2), km=(0.5, 0.5), resample=False).to_c()
    assert list(c.mass) == pytest.approx([0.8, 1.2]) and list(c.km) == [0.5, 0.5] and c.resample == 0 and c.reserved == 0
    assert pkg.DynamicsRandomization.from_c(c).mass == pytest.approx((0.8, 1.2))
