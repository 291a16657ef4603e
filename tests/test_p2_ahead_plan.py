"""Host side of the persistent SGHMC look-ahead (csrc/hmcx_persist2.hip: p2_ahead_mode, p2_layout with two
lanes, hmcx_p2_ahead_rule) through hmcx_p2_ahead_query and the rule itself — host arithmetic only, no
device."""
import ctypes

import pytest

REGIONS = ("XA", "XD", "XB", "XW", "XS", "XC", "XQ", "L1", "XV")
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from dropout_hamiltonian_montecarlo_amd import _native
    return _native.load_library()


@pytest.fixture(scope="module")
def query(lib):
    def q(B, D, K, tsize=8, num_cus=256, lds_max=LDS_CU, pad=1, want=1):
        out = (ctypes.c_longlong * 26)()
        assert lib.hmcx_p2_ahead_query(B, D, K, tsize, num_cus, lds_max, pad, want, out) == 0
        v = list(out)
        d = dict(zip(("ahead", "grid", "launch_lds", "lds"), v[:4]))
        d["regions"] = {name: (v[4 + 2 * i], v[5 + 2 * i]) for i, name in enumerate(REGIONS)}
        d["ngran"], d["Br"], d["BFP"], d["Ro"] = v[22:26]
        return d
    return q


@pytest.fixture(scope="module")
def plan(lib):
    def q(B, D, K, tsize=8, num_cus=256, lds_max=LDS_CU, pad=1, want=0):
        out = (ctypes.c_longlong * 31)()
        assert lib.hmcx_p2_plan_query(B, D, K, tsize, num_cus, lds_max, pad, want, out) == 0
        return list(out)
    return q


SHAPES = [(500, 784, 10), (40, 32, 10), (64, 49, 3), (100, 400, 12), (33, 17, 2), (16, 8, 10)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pad", [0, 1])
def test_two_lane_regions_are_disjoint_and_inside_the_arena(query, plan, shape, pad):
    p = query(*shape, pad=pad)
    assert p["ahead"] == 1
    end = 0
    for name in REGIONS:                                   # declaration order is address order
        off, size = p["regions"][name]
        assert off >= end and size > 0, name
        end = off + size
    assert end <= p["ngran"] and p["ngran"] * 16 < 2 ** 31
    r = p["regions"]
    # lane 1's copy of the five round regions: the same sizes in the same order, so one offset serves all
    assert r["L1"][1] == sum(r[n][1] for n in ("XA", "XD", "XB", "XW", "XS")) == r["XC"][0] - r["XA"][0]
    v = plan(*shape, pad=pad)
    Gr, Gf, Fo = v[1], v[2], v[7]
    G, KC = Gr * Gf, 10 if shape[2] == 10 else 16
    assert p["grid"] == 2 * G
    assert r["XQ"][1] >= 2 * G * (Fo * KC + KC)             # a slot per lane: slice + bias of every member
    assert r["XV"][1] == 2 * G * 8                          # a verdict line per workgroup and lane
    # lane 0's regions are where the plain launch has them
    for i, name in enumerate(("XA", "XD", "XB", "XW", "XS", "XC")):
        assert r[name] == (v[12 + 2 * i], v[13 + 2 * i])


def test_config2_lds_holds_two_tiles_within_a_cu(query):
    """Config 2 (8x16, 64 x 65 tile of doubles): the second tile and label block on top of the plan's LDS,
    within a CU's 160 KB and above half of it, so that no two workgroups share a CU."""
    p = query(500, 784, 10)
    assert (p["ahead"], p["grid"]) == (1, 256)
    assert (p["Br"], p["BFP"], p["Ro"]) == (64, 65, 4)
    assert p["launch_lds"] >= p["lds"] + 8 * (64 * 65 + 4 * 16)
    assert 2 * p["launch_lds"] > LDS_CU >= p["launch_lds"]


def test_off_leaves_the_launch_as_it_was(query, plan):
    p, v = query(500, 784, 10, want=0), plan(500, 784, 10)
    assert (p["ahead"], p["grid"], p["launch_lds"]) == (0, 128, p["lds"])
    assert p["regions"]["L1"][1] == 0 and p["regions"]["XV"][1] == 0 and p["regions"]["XQ"][1] == 0
    assert p["ngran"] == v[30]


@pytest.mark.parametrize("num_cus", [128, 255])
def test_fallback_when_twice_the_workgroups_do_not_fit(query, num_cus):
    p = query(500, 784, 10, num_cus=num_cus)
    assert (p["ahead"], p["grid"]) == (0, 128) and p["launch_lds"] == p["lds"]


def test_fallback_when_the_second_tile_does_not_fit(query):
    """An LDS that holds the plan (81 KB at config 2) but not the second 33 KB tile on top of it."""
    p = query(500, 784, 10, lds_max=100 * 1024)
    assert p["lds"] <= 100 * 1024 < p["lds"] + 8 * 64 * 65
    assert (p["ahead"], p["grid"], p["launch_lds"]) == (0, 128, p["lds"])


def test_fallback_when_the_state_gather_is_too_wide(query, plan):
    """B = 300, D = 1500, K = 10 (8x16, 12 owned features): a lane gathers the accepted state of its feature
    team with at most 4 granules per thread, 1,024 per workgroup, and 8 x (12 x 10 + 10) = 1,040 do not fit."""
    v = plan(300, 1500, 10)
    assert v[1] * (v[7] * 10 + 10) > 4 * 256
    p = query(300, 1500, 10)
    assert (p["ahead"], p["grid"], p["launch_lds"]) == (0, v[1] * v[2], p["lds"])


def test_auto_rule_transitions(lib):
    rule = lib.hmcx_p2_ahead_rule
    # fewer than 16 resolved steps decide nothing, whatever they say
    for seen in (0, 1, 15):
        assert rule(1, seen, seen) == 1 and rule(0, seen, 0) == 0
    # on: stays on up to an accept rate of 0.4, goes off above it
    assert rule(1, 16, 1) == 1 and rule(1, 32, 3) == 1            # the benchmark's ~9 %
    assert rule(1, 20, 8) == 1                                    # 0.4 exactly: not above
    assert rule(1, 32, 13) == 0 and rule(1, 16, 16) == 0
    # off: stays off down to 0.3, comes back below it
    assert rule(0, 32, 13) == 0 and rule(0, 20, 6) == 0           # 0.3 exactly: not below
    assert rule(0, 32, 9) == 1 and rule(0, 16, 0) == 1
    # hysteresis: between the thresholds the mode is the one it was
    for acc in range(10, 13):                                     # 0.31 … 0.375 of 32
        assert rule(1, 32, acc) == 1 and rule(0, 32, acc) == 0
