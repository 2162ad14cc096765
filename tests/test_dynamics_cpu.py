"""Dynamics randomisation (include/dronenav.h dn_enable_dynamics) without a GPU: the C struct against its ctypes twin, the exported
symbols, and the host-side validation of DynamicsRandomization."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

NEW_SYMBOLS = ("dn_enable_dynamics", "dn_set_dynamics", "dn_get_dynamics", "dn_get_dynamics_config")


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    return p


def test_dynamics_config_layout_matches_header(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dronenav.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(dn_dynamics_config), offsetof(dn_dynamics_config, mass),
           offsetof(dn_dynamics_config, inertia), offsetof(dn_dynamics_config, kf), offsetof(dn_dynamics_config, km),
           offsetof(dn_dynamics_config, resample), offsetof(dn_dynamics_config, reserved), DN_ABI_VERSION);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "dyn.c"), os.path.join(td, "dyn")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    D = pkg._capi.DnDynamicsConfig
    assert got == [C.sizeof(D), D.mass.offset, D.inertia.offset, D.kf.offset, D.km.offset, D.resample.offset, D.reserved.offset,
                   pkg._capi.ABI_VERSION], got
    assert C.sizeof(D) == 40 and pkg._capi.ABI_VERSION == 10            # additive: the ABI version stays


def test_dynamics_symbols_are_exported_and_bound(pkg):
    lib = pkg._capi.load()
    for name in NEW_SYMBOLS:
        assert name in pkg._capi.PROTOTYPES, name
        assert getattr(lib, name).argtypes == pkg._capi.PROTOTYPES[name][1], name
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._capi.library_path()]).decode()
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in out, name


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
