"""The MLP's dropout keep law for any ratio (csrc/hmcx_keep_law.h) on the CPU: a stand-alone C++ program, built with
the host compiler, prints keep_group's flags at seven ratios and what keep_law_of — the function behind
hmcx_set_mlp_dropout — answers for valid and invalid ratios.  The flags are compared with the host twins of
tests/_mlp_dropout.py (per-byte compares from the definition), with the constants-only law of ratio 0.1 and, where
the threshold's low 16 bits are zero, with closed forms on the element's top byte that share nothing with the twins'
tie handling.  The model's ``dropout=`` keyword is checked without a device."""
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _mlp_dropout as md

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dropout_hamiltonian_montecarlo_amd", "csrc")
EINVAL = -1
MSG = "mlp dropout: ratio must satisfy 0 <= ratio and ceil(ratio * 2^24) < 2^24"

# one (seed, chain, step, slot); the seed was fixed after the twin alone passed the kept-fraction bound below for it
SEED, CHAIN, STEP, SLOT = 0x5EED0D1CE5, 3, 41, 0x80000007
NG = 6000                                                          # 384,000 flags
N3 = 64 * NG
VALID = [("-0.0", -0.0), ("0.0", 0.0), ("1.0 - 1.0 / 16777216.0", 1.0 - 2.0 ** -24), ("0.1", 0.1), ("0.05", 0.05),
         ("0.9", 0.9)]
INVALID = [("1.0", 1.0), ("1.5", 1.5), ("-1e-9", -1e-9), ("NAN", float("nan")), ("INFINITY", float("inf"))]

PROGRAM = r"""
#include "hmcx_keep_law.h"
#include <cstdio>
#include <cmath>
using namespace hmcx;

static void flags(double ratio) {
  KeepLaw law; double scale; const char* msg = nullptr;
  if (keep_law_of(ratio, &law, &scale, &msg) != HMCX_OK) { std::printf("F %%.17g failed\n", ratio); return; }
  std::printf("F %%.17g", ratio);
  for (uint32_t G = 0; G < %(ng)du; ++G) {
    const KeepGroup k = keep_group(law, %(seed)dull, G, %(slot)du, %(step)du, %(chain)du);
    std::printf(" %%08x%%08x", k.hi, k.lo);
  }
  std::printf("\n");
}
static void default_flags() {                                     // the constants-only law type the hot kernels keep
  std::printf("D");
  for (uint32_t G = 0; G < %(ng)du; ++G) {
    const KeepGroup k = keep_group(KeepLawDefault{}, %(seed)dull, G, %(slot)du, %(step)du, %(chain)du);
    std::printf(" %%08x%%08x", k.hi, k.lo);
  }
  std::printf("\n");
}
static void law(const char* name, double ratio) {
  KeepLaw l = {0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu};
  double scale = -7.0;
  const char* msg = "";
  const int rc = keep_law_of(ratio, &l, &scale, &msg);
  std::printf("L\t%%s\t%%d\t%%s\t%%08x\t%%08x\t%%04x\t%%a\n", name, rc, msg, l.tb4, l.add, l.tl, scale);
}

int main() {
  const double ratios[] = {%(ratios)s};
  for (double r : ratios) flags(r);
  default_flags();
%(laws)s
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("mlp_dropout")
    src, exe = d / "law.cpp", d / "law"
    laws = "\n".join('  law("%s", %s);' % (n, n) for n, _ in VALID + INVALID)
    src.write_text(PROGRAM % dict(ng=NG, seed=SEED, slot=SLOT, step=STEP, chain=CHAIN,
                                  ratios=", ".join(repr(r) for r in md.RATIOS), laws=laws))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(REPO, "include"), "-I", CSRC,
            str(src), "-o", str(exe)]
    # the sanitizers where their runtimes link (statically: nothing to preload); the plain program otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    flags, laws = {}, {}
    for line in r.stdout.splitlines():
        if line.startswith("D "):
            line = "F default " + line[2:]
        if line.startswith("F "):
            parts = line.split(" ")
            assert len(parts) == 2 + NG, parts[:3]
            words = np.array([int(w, 16) for w in parts[2:]], dtype=np.uint64)             # hi:lo, element p = bit p
            bits = (words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
            flags[parts[1] if parts[1] == "default" else float(parts[1])] = bits.astype(bool).reshape(-1)
        elif line.startswith("L\t"):
            _, name, rc, msg, tb4, add, tl, scale = line.split("\t")
            laws[name] = (int(rc), msg, int(tb4, 16), int(add, 16), int(tl, 16), float.fromhex(scale))
    return flags, laws


@pytest.fixture(scope="module")
def top_bytes():
    return md.group_bytes(SEED, N3, SLOT, STEP, CHAIN).reshape(-1)


def test_headers_need_no_hip():
    """hmcx_keep_law.h and hmcx_philox.h include the HIP runtime only under the device compiler."""
    for name, want in (("hmcx_keep_law.h", ['"hmcx.h"', '"hmcx_philox.h"', "<math.h>"]),
                       ("hmcx_philox.h", ["<stdint.h>", "<hip/hip_runtime.h>"])):
        with open(os.path.join(CSRC, name)) as fh:
            assert [ln.split()[1] for ln in fh if ln.startswith("#include")] == want


@pytest.mark.parametrize("ratio", md.RATIOS)
def test_keep_group_equals_the_twin(program, ratio):
    flags, _ = program
    want = md.keep_group_host(ratio, SEED, N3, SLOT, STEP, CHAIN)
    assert flags[ratio].shape == want.shape == (N3,) and N3 >= 384000
    np.testing.assert_array_equal(flags[ratio], want)


def test_default_ratio_is_the_constants_only_law(program):
    flags, _ = program
    want = md.keep_group_host_default(SEED, N3, SLOT, STEP, CHAIN)
    np.testing.assert_array_equal(flags[0.1], want)
    np.testing.assert_array_equal(flags["default"], want)          # KeepLawDefault: the constants k_fwdr's rows keep
    byte = md.group_bytes(SEED, N3, SLOT, STEP, CHAIN)
    assert (byte == 0x19).sum() > 1000                             # the ties the comparison is about


def test_closed_forms_where_the_low_bits_are_zero(program, top_bytes):
    """tl == 0: the flag is a function of the element's top byte alone."""
    flags, _ = program
    np.testing.assert_array_equal(flags[0.5], (top_bytes >> 7) & 1 == 1)
    np.testing.assert_array_equal(flags[0.25], top_bytes >= 0x40)
    np.testing.assert_array_equal(flags[0.75], top_bytes >= 0xC0)
    assert flags[0.0].all()
    for r, tb in ((0.5, 0x80), (0.25, 0x40), (0.75, 0xC0), (0.0, 0x00)):
        assert (top_bytes == tb).sum() > 1000                      # ties occur, and every one keeps


@pytest.mark.parametrize("ratio", md.RATIOS)
def test_kept_fraction(program, ratio):
    """Within 5 sigma of 1 - r over n flags (the twin alone passes this for the seed: asserted first)."""
    flags, _ = program
    n = N3
    bound = 5.0 * math.sqrt(ratio * (1.0 - ratio) / n)
    twin = md.keep_group_host(ratio, SEED, N3, SLOT, STEP, CHAIN).mean()
    got = flags[ratio].mean()
    print("ratio %.2f: kept %.6f (twin %.6f), want %.6f +- %.6f" % (ratio, got, twin, 1.0 - ratio, bound))
    assert abs(twin - (1.0 - ratio)) <= bound
    assert abs(got - (1.0 - ratio)) <= bound


def test_validation_and_thresholds(program):
    _, laws = program
    for name, r in VALID:
        rc, msg, tb4, add, tl, scale = laws[name]
        t = md.threshold(r)
        assert rc == 0 and msg == "", (name, rc, msg)
        assert tb4 == (t >> 16) * 0x01010101 and tl == t & 0xFFFF, name
        assert add == (0x7F - ((t >> 16) & 0x7F)) * 0x01010101, name
        assert scale == 1.0 / (1.0 - r), name
    for name, _ in INVALID:                                        # EINVAL, the message, the outputs untouched
        assert laws[name] == (EINVAL, MSG, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF, -7.0), (name, laws[name])
    assert md.threshold(0.1) == 0x19999A and laws["0.1"][2:5] == (0x19191919, 0x66666666, 0x999A)
    assert md.threshold(0.05) == 0xCCCCD and laws["0.05"][2:5] == (0x0C0C0C0C, 0x73737373, 0xCCCD)
    assert md.threshold(0.9) == 0xE66667 and laws["0.9"][2:5] == (0xE6E6E6E6, 0x19191919, 0x6667)
    assert laws["0.1"][5] == 1.0 / 0.9                             # today's scale, bit for bit
    assert laws["1.0 - 1.0 / 16777216.0"][2:5] == (0xFFFFFFFF, 0x00000000, 0xFFFF)


def test_python_rule_matches(program):
    """_native.mlp_dropout_threshold: the same thresholds, ValueError where keep_law_of says EINVAL."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    for _, r in VALID:
        assert nat.mlp_dropout_threshold(r) == md.threshold(r)
    for _, r in INVALID:
        with pytest.raises(ValueError, match="mlp dropout"):
            nat.mlp_dropout_threshold(r)


def test_model_keyword_without_a_device(monkeypatch):
    """mlp(..., dropout=r) stores the ratio; an invalid one raises ValueError before any context is asked for."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu import mlp as mlp_mod
    asked = []

    def no_device(device=None):
        asked.append(device)
        return types.SimpleNamespace(device="cpu")
    monkeypatch.setattr(mlp_mod, "context", no_device)
    for _, r in INVALID:
        with pytest.raises(ValueError, match="mlp dropout"):
            mlp_mod.mlp({"alpha": 0.01}, 4, 8, 2, dropout=r)
    assert asked == []
    assert mlp_mod.mlp({"alpha": 0.01}, 4, 8, 2).dropout == 0.1
    for r in (0.0, 0.5, 0.9, 1.0 - 2.0 ** -24):
        assert mlp_mod.mlp({"alpha": 0.01}, 4, 8, 2, dropout=r).dropout == r
    assert len(asked) == 5


def test_context_helper_sets_the_models_ratio(monkeypatch):
    """mlp_context makes the shared context's ratio the calling model's, the default for a model that names none;
    the samplers reach the same function through _mlp_call."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu import mlp as mlp_mod
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu import _mlp_call
    assert _mlp_call.mlp_context is mlp_mod.mlp_context
    sets = []
    ctx = types.SimpleNamespace(set_mlp_dropout=sets.append)
    monkeypatch.setattr(mlp_mod, "context", lambda device=None: ctx)
    a, b = types.SimpleNamespace(device="cpu", dropout=0.5), types.SimpleNamespace(device="cpu")
    for m in (a, b, a, b):
        assert mlp_mod.mlp_context(m) is ctx
    assert sets == [0.5, 0.1, 0.5, 0.1]
