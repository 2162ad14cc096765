"""The track bank (include/dronenav.h dn_enable_tracks) without a GPU: what TrackBank refuses on the CPU, the configuration it hands the
C ABI, the struct's layout against the header, and the cdf / draw statement on hand cases."""

import numpy as np
import pytest

import abi_support as abi
from drl_dronenavigation_amd import Track, TrackBank, _capi, tracks



def test_trackbank_refuses_what_the_library_refuses():
    up, fwd = tracks.up(), tracks.half_up_forward()
    bank = TrackBank([up, fwd])
    assert len(bank) == 2 and bank.resample and bank.num_waypoints == [5, 3] and np.array_equal(bank.weights, [1, 1])
    with pytest.raises(ValueError, match="1..64 tracks"):
        TrackBank([])
    with pytest.raises(ValueError, match="1..64 tracks"):
        TrackBank([Track([[0, 0, 1]], up.initial_xyzs, up.aviary_dim)] * 65)
    with pytest.raises(TypeError):
        TrackBank([up, "fwd"])
    with pytest.raises(ValueError, match="circle"):
        TrackBank([up, tracks.circle(1, 4, 1)])
    with pytest.raises(ValueError, match="initial_xyzs or aviary_dim"):
        TrackBank([up, tracks.reaching()])
    with pytest.raises(ValueError, match="initial_xyzs or aviary_dim"):
        TrackBank([up, Track(fwd.waypoints, [[0, 0, .2]], fwd.aviary_dim)])
    with pytest.raises(ValueError, match="at most 64"):
        TrackBank([tracks.up_circle()] * 6)                                   # 72 waypoints in all
    assert len(TrackBank([tracks.up_circle()] * 5 + [Track(np.zeros((4, 3)), up.initial_xyzs, up.aviary_dim)])) == 6      # exactly 64
    with pytest.raises(ValueError, match="no waypoints"):
        TrackBank([up, Track(np.zeros((0, 3)), up.initial_xyzs, up.aviary_dim)])
    with pytest.raises(ValueError, match="not finite"):
        TrackBank([up, Track([[0, 0, np.nan]], up.initial_xyzs, up.aviary_dim)])
    for w in ([1, -1], [1, np.inf], [np.nan, 1]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            TrackBank([up, fwd], weights=w)
    with pytest.raises(ValueError, match="every weight is zero"):
        TrackBank([up, fwd], weights=[0, 0])
    with pytest.raises(ValueError, match="one value per track"):
        TrackBank([up, fwd], weights=[1, 2, 3])


def test_to_c_concatenates_the_tracks_and_round_trips():
    up, fwd, one = tracks.up(), tracks.half_up_forward(), Track([[0, 0, .3]], [[0, 0, .1]], tracks.up().aviary_dim)
    bank = TrackBank([up, fwd, one], weights=[1, 0, 2.5], resample=False)
    c = bank.to_c()
    assert c.num_tracks == 3 and list(c.num_waypoints[:4]) == [5, 3, 1, 0] and c.resample == 0 and c.reserved == 0
    assert np.array_equal(np.array(c.waypoints[:27]).reshape(9, 3), np.vstack([up.waypoints, fwd.waypoints, one.waypoints]))
    assert list(c.weight[:4]) == [1.0, 0.0, 2.5, 0.0]
    back = TrackBank.from_c(c, up.initial_xyzs, up.aviary_dim)
    assert back.num_waypoints == [5, 3, 1] and not back.resample and np.array_equal(back.weights, bank.weights)
    assert all(np.array_equal(a.waypoints, b.waypoints) for a, b in zip(back.tracks, bank.tracks))


def test_struct_layout_matches_the_header():
    abi.check_layout(_capi.DnTrackBankConfig, 2064, num_waypoints=4, waypoints=264, weight=1800, resample=2056, reserved=2060)   # the layout line of the header's comment
    assert abi.compiled().constants["DN_MAX_TRACKS"] == _capi.MAX_TRACKS == 64
    abi.check_version()


def test_cdf_and_draw_on_hand_cases():
    """cdf_k = S_k / S_{T-1} on float64 partial sums of the float32 weights; t = #{k in 0..T-2 : u >= cdf_k}."""
    t = [Track([[0, 0, .3 + .1 * k]], [[0, 0, .1]], tracks.up().aviary_dim) for k in range(6)]
    bank = TrackBank(t, weights=[1, 0, 2, 1, 3, 1])                           # a zero weight in the middle
    cdf = bank.cdf()
    assert cdf.dtype == np.float64 and np.array_equal(cdf, np.array([1, 1, 3, 4, 7, 8]) / 8.0)
    u = np.array([0.0, 0.124999, 0.125, 0.3, 0.375, 0.4999, 0.5, 0.874999, 0.875, 1.0 - 2.0 ** -33])
    assert TrackBank.draw(cdf, u).tolist() == [0, 0, 2, 2, 3, 3, 4, 4, 5, 5]  # u AT a boundary belongs to the next track; 1 is never drawn
    # zero weights at the end: the last cdf entries repeat 1, and u < 1 never reaches them
    cdf = TrackBank(t[:4], weights=[2, 2, 0, 0]).cdf()
    assert np.array_equal(cdf, [0.5, 1.0, 1.0, 1.0])
    assert TrackBank.draw(cdf, [0.0, 0.5 - 2.0 ** -33, 0.5, 1.0 - 2.0 ** -33]).tolist() == [0, 0, 1, 1]
    # ... and at the start
    cdf = TrackBank(t[:3], weights=[0, 0, 5]).cdf()
    assert TrackBank.draw(cdf, [0.5 / 2 ** 32, 0.3, 1.0 - 2.0 ** -33]).tolist() == [2, 2, 2]
    # the smallest and largest u the draw can form, (r + 0.5) / 2^32 for r = 0 and 2^32 - 1, and weights that are no binary fractions:
    # the partial sums are those of the float32 values, in float64
    w = np.array([0.1, 0.2, 0.3], np.float32)
    cdf = TrackBank(t[:3], weights=w).cdf()
    s = np.cumsum(w.astype(np.float64))
    assert np.array_equal(cdf, s / s[-1]) and cdf[-1] == 1.0
    assert TrackBank.draw(cdf, [0.5 / 2 ** 32, (2.0 ** 32 - 0.5) / 2 ** 32]).tolist() == [0, 2]
    # one track: nothing to compare with
    assert TrackBank.draw(TrackBank(t[:1]).cdf(), [0.0, 0.9]).tolist() == [0, 0]
