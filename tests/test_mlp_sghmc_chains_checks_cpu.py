"""The argument checks of hmcx_mlp_sghmc_chains_run (csrc/hmcx_mlp_checks.h, sghmc_chains) on the CPU, by the recipe
of tests/test_mlp_checks_cpu.py: a stand-alone C++ program with its own main, built with the host compiler and, where
their runtimes link, the address and undefined-behaviour sanitizers, runs every row of the table below and prints
status and message.  The per-step arrays are heap blocks of exactly n_steps (3) or n_steps * C (6) entries with the
defect in the last one, so a scan that read past an array would fail the run.  CASES is what the GPU test replays
against the entry point itself (tests/test_gpu_mlp_sghmc_chains.py)."""
import os
import shutil
import subprocess

import pytest

import test_mlp_checks_cpu as base

WHO = "mlp sghmc chains: "
OK, EINVAL, EUNSUP = base.OK, base.EINVAL, base.EUNSUP

ROWS = [
    ("valid", "", OK, ""),
    ("null args", "sghmc_chains(nullptr)", EINVAL, "null args"),
    ("n_steps 0", "a.n_steps = 0;", OK, ""),
    ("n_steps < 0", "a.n_steps = -1;", EINVAL, WHO + "n_steps < 0"),
    ("dtype", "a.dtype = 2;", EINVAL, base.DTYPE),
    ("sizes", "a.B = 0;", EINVAL, base.SIZES),
    ("C 0", "a.C = 0;", EINVAL, WHO + "C must be 1 .. 64"),
    ("C 65", "a.C = 65;", EINVAL, WHO + "C must be 1 .. 64"),
    ("order repeats", "a.order[0] = a.order[1];", EINVAL, WHO + "order must be a permutation of 0..5"),
    ("order out of range", "a.order[5] = 6;", EINVAL, WHO + "order must be a permutation of 0..5"),
    ("n_iter < 0 in the last entry", "b.iters.back() = -1;", EINVAL, WHO + "n_iter < 0"),
    ("n_iter wraps the forward number", "b.iters.back() = 357913941;", EINVAL,
     WHO + "n_iter so large that the forward number wraps 2^32"),
    ("the largest n_iter", "b.iters.back() = 357913940;", OK, ""),
    ("chain0 + C wraps", "a.chain0 = 0xffffffffu;", EINVAL, WHO + "chain0 + C wraps 2^32"),
    ("chain0 + C reaches 2^32", "a.chain0 = 0xfffffffeu;", OK, ""),
    ("step_base + n_steps wraps", "a.step_base = 0xfffffffeu;", EINVAL, WHO + "step_base + n_steps wraps 2^32"),
    ("draw_stride below the flagged steps", "a.draw_stride = 2;", EINVAL, WHO + "draw_stride below the call's flagged steps"),
    ("want_draw without draws", "a.draws.p[4] = nullptr;", EINVAL, WHO + "want_draw needs draws"),
    ("BUFFER noise without noise_off", "a.noise_off = nullptr;", EINVAL, WHO + "BUFFER noise mode needs noise and noise_off"),
    ("BUFFER noise without noise", "a.noise = nullptr;", EINVAL, WHO + "BUFFER noise mode needs noise and noise_off"),
    ("FIXED masks without mask_off", "a.mask_off = nullptr;", EINVAL, WHO + "FIXED masks need masks and mask_off"),
    ("FIXED masks without masks", "a.masks = nullptr;", EINVAL, WHO + "FIXED masks need masks and mask_off"),
    ("PHILOX modes read neither offset array",
     "a.noise_mode = HMCX_NOISE_PHILOX; a.noise_off = nullptr; a.mask_mode = HMCX_MLP_MASKS_PHILOX; a.mask_off = nullptr;",
     OK, ""),
    ("NONE masks need no buffer", "a.mask_mode = HMCX_MLP_MASKS_NONE; a.masks = nullptr; a.mask_off = nullptr;", OK, ""),
    ("bad noise_mode", "a.noise_mode = 2;", EINVAL, WHO + "bad noise_mode"),
    ("bad mask_mode", "a.mask_mode = 3;", EINVAL, WHO + "bad mask_mode"),
    ("null row0", "a.row0 = nullptr;", EINVAL, WHO + "null pointer"),
    ("null n_iter", "a.n_iter = nullptr;", EINVAL, WHO + "null pointer"),
    ("null out_loss", "a.out_loss = nullptr;", EINVAL, WHO + "null pointer"),
    ("hole in par", "a.par.p[3] = nullptr;", EINVAL, WHO + "null pointer"),
    ("out_nlp and out_E are optional", "a.out_nlp = nullptr; a.out_E = nullptr;", OK, ""),
    ("negative row0 in the last step", "b.row0.back() = -1;", EINVAL, WHO + "negative row0"),
    ("negative noise_off in the last entry", "b.coff.back() = -1;", EINVAL, WHO + "negative noise_off"),
    ("negative mask_off in the last entry", "b.cmoff.back() = -1;", EINVAL, WHO + "negative mask_off"),
    ("2^31 parameters", "a.n_in = 46000; a.n_mid = 46000;", EUNSUP, WHO + "more than 2^31 - 1 parameters"),
    ("C before order", "a.C = 0; a.order[0] = 9;", EINVAL, WHO + "C must be 1 .. 64"),
    ("the scan before draw_stride", "b.iters.back() = -1; a.draw_stride = 0;", EINVAL, WHO + "n_iter < 0"),
]

VALID = r"""
static hmcx_mlp_sghmc_chains_args valid_sghmc_chains(Bufs& b) {
  hmcx_mlp_sghmc_chains_args a{}; dims(a); order(a); a.n_steps = NS; a.C = NC; a.X = P; a.y = Y;
  a.row0 = b.row0.data(); a.eps = b.eps.data(); a.n_iter = b.iters.data(); a.u_accept = b.u.data();
  a.noise_mode = HMCX_NOISE_BUFFER; a.noise = PD; a.noise_off = b.coff.data();
  a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = P; a.mask_off = b.cmoff.data();
  a.par = PAR; a.out_A = PD; a.out_accepted = Y; a.out_loss = PD; a.out_nlp = PD; a.out_E = PD;
  a.want_draw = b.draw.data(); a.draws = PAR; a.draw_stride = NS;
  return a;
}
"""


def _program():
    head, main = base.PROGRAM_HEAD.rsplit("int main() {", 1)
    body = []
    for i, (_case, code, _st, _msg) in enumerate(ROWS):
        if code.endswith("(nullptr)"):
            body.append("  report(%d, %s);" % (i, code))
        else:
            body.append("  { Bufs b; auto a = valid_sghmc_chains(b); %s report(%d, sghmc_chains(&a)); }" % (code, i))
    return head + VALID + "int main() {" + main + "\n".join(body) + "\n  return 0;\n}\n"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("mlp_sghmc_chains_checks")
    src, exe = d / "checks.cpp", d / "checks"
    src.write_text(_program())
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(base.REPO, "include"), "-I", base.CSRC,
           str(src), "-o", str(exe)]
    # the sanitizers where their runtimes link (statically: nothing to preload); the plain program otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        row, status, msg = line.split("\t")
        got[int(row)] = (int(status), msg)
    return got


def test_table_names_every_case_once():
    assert len({r[0] for r in ROWS}) == len(ROWS)
    for case in ("valid", "n_steps 0", "C 0", "C 65", "order repeats", "n_iter < 0 in the last entry", "chain0 + C wraps",
                 "draw_stride below the flagged steps", "BUFFER noise without noise_off", "FIXED masks without mask_off"):
        assert any(r[0] == case for r in ROWS), case


def test_every_row_gives_the_status_and_message(results):
    assert sorted(results) == list(range(len(ROWS)))
    bad = [(ROWS[i][0], results[i], ROWS[i][2:]) for i in range(len(ROWS)) if results[i] != tuple(ROWS[i][2:])]
    assert not bad, bad
