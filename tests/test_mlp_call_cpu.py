"""The host plumbing the dropout MLP's callers share (inference/gpu/_mlp_call.py, hmc._assemble_chains) without a
device: the mask plan against a recording provider, negative_log_posterior from evaluation pieces bit for bit
against mlp.nlp_from_parts, and the per-chain assembly against what hmc._chains_fused printed and returned for the
same phase outputs before the assembly became a function (tests/golden/assemble_chains.json)."""
import io
import json
import os
import types

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assemble_chains.json")


# ---------------------------------------------------------------------------------------------- mask_plan
class Recorder:
    def __init__(self, B, n_mid, shape=None):
        self.calls, self.B, self.n_mid, self.shape = [], B, n_mid, shape

    def __call__(self, step, nf):
        self.calls.append((step, nf))
        shape = self.shape or (nf, 3, self.B, self.n_mid)
        return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) + 1000.0 * step


def test_mask_plan_provider_calls_offsets_and_values():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu import _mlp_call
    B, n_mid, n3 = 2, 3, 18
    n_fwd = np.array([1, 3, 2, 1], dtype=np.uint8)
    rec = Recorder(B, n_mid)
    mode, host, mask_off, eval_off = _mlp_call.mask_plan(None, rec, 40, n_fwd, B, n_mid, "sgld(mlp)")
    assert mode == nat.MLP_MASKS_FIXED
    assert rec.calls == [(40, 1), (41, 3), (42, 2), (43, 1)]
    starts = np.array([0, 1, 4, 6]) * n3
    np.testing.assert_array_equal(mask_off, starts)
    np.testing.assert_array_equal(eval_off, np.stack([starts + n3, starts + 2 * n3], axis=1))
    assert mask_off.dtype == np.int64 and eval_off.dtype == np.int64 and eval_off.flags.c_contiguous
    want = np.concatenate([np.arange(nf * n3) + 1000.0 * (40 + s) for s, nf in enumerate(n_fwd)])
    np.testing.assert_array_equal(host, want)
    assert host.shape == (7 * n3,)


def test_mask_plan_off_and_philox_return_no_buffer():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu import _mlp_call
    rec = Recorder(2, 3)
    for arg, provider, mode in (('off', None, nat.MLP_MASKS_NONE), ('off', rec, nat.MLP_MASKS_NONE),
                                (None, None, nat.MLP_MASKS_PHILOX)):
        got = _mlp_call.mask_plan(arg, provider, 0, np.array([1, 2]), 2, 3, "sgd(mlp)")
        assert got[0] == mode and got[1] is None
        assert not got[2].any() and not got[3].any() and got[2].shape == (2,) and got[3].shape == (2, 2)
    assert rec.calls == []
    # no step: a provider is never called and there is nothing to upload
    assert _mlp_call.mask_plan(None, rec, 0, np.zeros(0, dtype=np.uint8), 2, 3, "sgd(mlp)")[1] is None


def test_mask_plan_errors_keep_their_messages():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu import _mlp_call
    for bad in ('on', 0, [np.ones((1, 2))]):
        with pytest.raises(ValueError) as e:
            _mlp_call.mask_plan(bad, None, 0, np.array([1]), 2, 3, "sgd(mlp)")
        assert str(e.value) == "masks must be None or 'off' (inject masks through mask_provider)"
    for who in ("sgd(mlp)", "sgld(mlp)"):
        with pytest.raises(HmcxError) as e:
            _mlp_call.mask_plan(None, Recorder(2, 3, shape=(2, 3, 2, 4)), 5, np.array([1, 2]), 2, 3, who)
        assert str(e.value) == who + ": mask_provider must return [1, 3, 2, 3]"


# ---------------------------------------------------------------------------------------------- nlp_from_eval
@pytest.mark.parametrize("axes", [(), (3,), (4, 3)])
def test_nlp_from_eval_equals_nlp_from_parts_bit_for_bit(axes):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu import _mlp_call
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES, mlp, mlp_param_shapes
    shapes = mlp_param_shapes(7, 5, 3)
    model = types.SimpleNamespace(alpha=0.037, shapes=shapes)
    keys = [MLP_PARAM_NAMES[i] for i in (4, 0, 5, 2, 1, 3)]                    # a start order that is not canonical
    start = {k: np.zeros(shapes[k]) for k in keys}
    rng = np.random.RandomState(11)
    loss = rng.standard_normal(axes) * 3.0
    sumsq = rng.standard_normal(axes + (6,)) ** 2 * 1e3
    got = _mlp_call.nlp_from_eval(model, keys, loss, sumsq)
    assert np.shape(got) == axes and np.asarray(got).dtype == np.float64
    want = np.empty(axes)
    for idx in np.ndindex(*axes):
        parts = [loss[idx]] + [sumsq[idx][MLP_PARAM_NAMES.index(k)] for k in keys]
        want[idx] = mlp.nlp_from_parts(model, parts, start)
    assert np.asarray(got).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- _assemble_chains
C, DIM = 2, 3
SCENARIOS = {"burn and draws": (20, 10), "no burn-in": (0, 10), "no draws": (20, 0)}


def _phase(n, record):
    """Synthetic outputs of one phase (hmc._mvn_phase's tuple): A, accepted, nlp, L [n, C], trace and momenta
    [n, C, DIM], the device trace."""
    rng = np.random.RandomState(100 + n + int(record))
    A = rng.uniform(0.05, 1.0, (n, C))
    tr = rng.standard_normal((n, C, DIM)) if record else None
    return (A, rng.uniform(size=(n, C)) < A, rng.standard_normal((n, C)) * 10, np.ceil(rng.uniform(0, 9, (n, C))),
            tr, rng.standard_normal((n, C, DIM)), tr)


def _jsonable(x):
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape), "values": [float(v) for v in x.reshape(-1)]}
    return x


def run_scenarios():
    """{scenario: (printed text, results, traces)} of hmc._chains_fused on the MVN route with the phases above in
    place of the device calls; the golden file holds what this returned before _assemble_chains existed."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    out = {}
    for name, (nburn, niter) in SCENARIOS.items():
        model = types.SimpleNamespace(_hmcx_model='mvn_gaussian', device='cpu')
        s = hmc(model, {'x': np.array([0.5, -1.5, 2.0])}, step_size=0.25)
        s.out = io.StringIO()
        s._mvn_phase = lambda st, n, C_, rngs, record: _phase(n, record)
        results, traces, _ = s._chains_fused(niter, nburn, C, None, None, nburn / 10)
        out[name] = _jsonable({"text": s.out.getvalue(), "results": results, "traces": traces})
    return out


def test_assemble_chains_prints_and_returns_what_chains_fused_did():
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    got = json.loads(json.dumps(run_scenarios()))
    assert sorted(got) == sorted(golden)
    for name in golden:
        assert got[name]["text"] == golden[name]["text"], name
        assert got[name]["traces"] == golden[name]["traces"], name
        assert got[name]["results"] == golden[name]["results"], name
    lines = golden["burn and draws"]["text"].splitlines()
    assert len(lines) == C * (10 + 1 + 10) and lines[10].startswith("adapted step size : ")
    assert golden["no draws"]["results"][0][1]["shape"] == [0]


def test_assemble_chains_without_momenta_leaves_the_lists_empty():
    """The MLP route's keep_momentum=False: momentum None, everything else as with momenta."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    with open(GOLDEN) as fh:
        golden = json.load(fh)["no burn-in"]
    s = hmc(types.SimpleNamespace(_hmcx_model='mvn_gaussian', device='cpu'), {'x': np.array([0.5, -1.5, 2.0])},
            step_size=0.25)
    s.out = io.StringIO()
    A, acc, nlp, L, tr, _, _ = _phase(10, True)
    x0 = np.array([0.5, -1.5, 2.0])
    results, traces = s._assemble_chains(C, 0, 10, None, None, (A, acc, L, nlp), lambda c: {'x': tr[:, c].copy()},
                                         lambda c, i: {'x': (x0 if i == 0 else tr[i - 1, c]).copy()}, None)
    assert [r[3] for r in results] == [[], []]
    got = json.loads(json.dumps(_jsonable({"text": s.out.getvalue(), "traces": traces,
                                           "results": [r[:3] for r in results]})))
    assert got["text"] == golden["text"] and got["traces"] == golden["traces"]
    assert got["results"] == [r[:3] for r in golden["results"]]


if __name__ == "__main__":                      # records the golden file: run against the code to be pinned
    with open(GOLDEN, "w") as fh:
        json.dump(run_scenarios(), fh)
