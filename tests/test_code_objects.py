"""CPU-side check of what each compile unit's device binary holds (no GPU): the kernel symbols of every gfx950
code object of the built library, read with tools/kernel_resources.py.  Symbol names only, no instructions.

A kernel that sits in two code objects is two device copies of one symbol, and which of them a launch runs is
decided by link order.  The MLP's multi-chain unit once held a second copy of 96 GEMM kernels that way
(DESIGN 5.3); it sees the shared launch helpers as prototypes only now, and this test keeps it so."""
import collections
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "dropout_hamiltonian_montecarlo_amd", "lib", "libhmcx.so")

# static kernels are unit-local: one harmless copy per unit that defines them.  The list may shrink, not grow.
UNIT_LOCAL = {"k_mlp_keep", "k_mlp_accept", "k_loss_final", "k_mlp_sgd_eval"}
CHAIN_OWN = {"k_mmc", "k_pending_chains", "k_mlp_sgld_chains"}


def _base(demangled):
    """'void hmcx::k_mm<float, 0>(hmcx::MMArgs<float>)' -> 'k_mm'"""
    head = demangled.split("(", 1)[0].split("<", 1)[0]
    return head.split()[-1].split("::")[-1]


@pytest.fixture(scope="module")
def objects():
    """Per code object: the base names of its kernels, and the mangled symbols."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    if not os.path.exists(kr.READELF):
        pytest.skip("llvm-readelf not found")
    pytest.importorskip("yaml")
    out = []
    for co in kr.code_objects(kr.fatbin(LIB)):
        syms = [k["symbol"][:-3] for k in kr.kernels(co)]
        out.append((syms, [_base(d) for d in kr.demangle(syms)]))
    assert len(out) >= 10 and sum(len(s) for s, _ in out) >= 400, [len(s) for s, _ in out]
    return out


def test_no_kernel_in_two_code_objects(objects):
    count = collections.Counter(s for syms, _ in objects for s in syms)
    base = {s: b for syms, names in objects for s, b in zip(syms, names)}
    dup = {base[s] for s, c in count.items() if c > 1}
    print("%d symbols, %d placements, in more than one code object: %s" % (len(count), sum(count.values()), sorted(dup)))
    assert dup <= UNIT_LOCAL, sorted(dup - UNIT_LOCAL)


def test_chain_units_hold_their_own_kernels_only(objects):
    chain = [set(names) for _, names in objects if "k_mlp_sgld_chains" in names]
    assert len(chain) == 2, len(chain)                       # one unit per dtype
    for names in chain:
        assert CHAIN_OWN <= names, sorted(names)
        assert names <= CHAIN_OWN | {"k_mlp_sgd_eval"}, sorted(names - CHAIN_OWN)


def test_kernel_resources_reports_copies(objects):
    """The tool says so when a symbol has several copies instead of printing one line for them."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), LIB, "--grep", "^$"],
                       capture_output=True, text=True, check=True)
    count = collections.Counter(s for syms, _ in objects for s in syms)
    want = sorted(c for c in count.values() if c > 1)
    got = sorted(int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("in ") and "code objects:" in ln)
    assert got == want, r.stdout
