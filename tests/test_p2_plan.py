"""Host side of the persistent SGHMC launch plan (csrc/hmcx_persist2.hip: plan_p2, p2_help_mode,
p2_layout) through hmcx_p2_plan_query — host arithmetic only, no device."""
import ctypes

import pytest

REGIONS = ("XA", "XD", "XB", "XW", "XS", "XC", "XAh", "XQ", "XP")
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def query():
    from dropout_hamiltonian_montecarlo_amd import _native
    lib = _native.load_library()

    def q(B, D, K, tsize=8, num_cus=256, lds_max=LDS_CU, pad=1, want=2):
        out = (ctypes.c_longlong * 31)()
        assert lib.hmcx_p2_plan_query(B, D, K, tsize, num_cus, lds_max, pad, want, out) == 0
        v = list(out)
        d = dict(zip(("ok", "Gr", "Gf", "Br", "Bf", "BfP", "Ro", "Fo", "lds", "help", "launch_lds", "grid"), v[:12]))
        d["regions"] = {name: (v[12 + 2 * i], v[13 + 2 * i]) for i, name in enumerate(REGIONS)}
        d["ngran"] = v[30]
        return d
    return q


SHAPES = [(500, 784, 10), (40, 32, 10), (64, 49, 3), (300, 1500, 10), (100, 400, 12), (33, 17, 2), (16, 8, 10)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("want", [0, 1, 2])   # 1 (E_current alone) is not built: no helpers
def test_arena_regions_are_disjoint_and_inside_the_arena(query, shape, pad, want):
    p = query(*shape, pad=pad, want=want)
    assert p["ok"] and p["help"] in ((0, 2) if want == 2 else (0,))
    end = 0
    for name in REGIONS:                                   # declaration order is address order
        off, size = p["regions"][name]
        assert off >= end and size >= 0, name
        end = off + size
    # the arena is allocated, and zeroed, as ngran granules: every region lies inside it
    assert end <= p["ngran"] and p["ngran"] * 16 < 2 ** 31
    G = p["Gr"] * p["Gf"]
    if p["help"]:
        KC = 10 if shape[2] == 10 else 16
        assert p["regions"]["XAh"][1] == p["regions"]["XA"][1]           # the helpers' own A-RS region
        assert p["regions"]["XQ"][1] >= 2 * G * (p["Fo"] * KC + KC)      # both parities, slice + bias
    else:
        assert p["regions"]["XAh"][1] == 0 and p["regions"]["XQ"][1] == 0
    assert p["regions"]["XP"][1] == p["regions"]["XQ"][1]          # p0 as q: slice + bias
    assert p["regions"]["XC"][1] == G + 2                  # 'done' granules, decision word, one spare


def test_helpers_off_leaves_the_launch_as_it_was(query):
    p = query(500, 784, 10, want=0)
    assert (p["Gr"], p["Gf"], p["help"], p["grid"], p["launch_lds"]) == (8, 16, 0, 128, p["lds"])
    q = query(500, 784, 10, want=2)
    for name in ("XA", "XD", "XB", "XW", "XS", "XC"):      # the chain's regions do not move
        assert q["regions"][name] == p["regions"][name]


def test_helpers_never_share_a_cu_with_a_chain_workgroup(query):
    """With helpers the launch has 2·G workgroups and asks for more than half of a CU's LDS."""
    p = query(500, 784, 10, want=2)
    assert (p["help"], p["grid"]) == (2, 256)
    assert 2 * p["launch_lds"] > LDS_CU >= p["launch_lds"] >= p["lds"]


@pytest.mark.parametrize("num_cus", [128, 255])
def test_fallback_when_twice_the_workgroups_do_not_fit(query, num_cus):
    """2·G = 256 workgroups at one per CU do not fit a device of fewer CUs: the plan is the same 8x16
    one and the launch is today's helper-less one (same grid, same LDS, no helper regions), whatever
    HMCX_P2_HELP asks for."""
    p, q = query(500, 784, 10, num_cus=num_cus, want=2), query(500, 784, 10, num_cus=num_cus, want=0)
    assert p == q and (p["help"], p["grid"]) == (0, 128)


def test_fallback_when_a_cu_cannot_be_claimed_whole(query):
    """A plan that needs all of a small LDS cannot ask for more than half of it plus the margin."""
    p = query(40, 32, 10, lds_max=24 * 1024, want=2)
    if p["ok"]:
        assert p["launch_lds"] <= 24 * 1024
        assert p["help"] == 0 or 2 * p["launch_lds"] > 24 * 1024
