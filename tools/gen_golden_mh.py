#!/usr/bin/env python3
"""Generate the random-walk Metropolis fixtures tests/golden/mh_{softmax,logistic,mvn}.npz by running the
REFERENCE's own sampler (hamiltonian/inference/cpu/metropolis.py, class MH) in a child process, against
the reference's own softmax / logistic / mvn_gaussian CPU models.

Run once where the reference checkout exists (HMCX_REFERENCE, default /root/reference):
    python tools/gen_golden_mh.py
The tests never run it; the committed .npz files (arrays only) travel instead.

Shim: as oracle/gen_golden.py (collections.Iterable, h5py, np.int / np.float), plus the reference's
``hamiltonian`` folder on sys.path so that metropolis.py's ``from utils import *`` resolves, and a no-op
tqdm when that package is absent.  The reference code path is not modified: per-step energies are
observed through the ``logp`` callable the sampler is given (metropolis.py:40-41 evaluates the proposal,
then the current state), the accept uniforms are the seeded global stream's (the sampler is its only
consumer), and the flags follow as ``isfinite(A) and u < A`` — cross-checked against which draws moved.

Configurations (global seed 0, chain from RandomState(0), C = 1):
  softmax  alpha 0.01, oracle.inputs.dataset(3, 60, 24, 10), zero start, 8 + 12 steps:
           'seq'  scale 0.1 update_sequential=True;  'site'  scale 0.5 update_sequential=False
  logistic alpha 0.25, logistic_inputs(3, 77, 33), zero start weights (33, 1) / bias (1,), scale 0.05, 8 + 12
  mvn      mu 0, cov [[1, .8], [.8, 1]]: 'near' start 0, scale 1, 50 + 200;  'far' start (60, -60), scale 30, 0 + 40
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden')
REFERENCE = os.environ.get('HMCX_REFERENCE', '/root/reference')

CHILD = r'''
import sys, types, collections, collections.abc, io, contextlib, importlib.util
sys.dont_write_bytecode = True
REF = sys.argv[3]
sys.path.insert(0, REF)
sys.path.insert(0, REF + '/hamiltonian')
collections.Iterable = collections.abc.Iterable
sys.modules.setdefault('h5py', types.ModuleType('h5py'))
try:
    import tqdm  # noqa: F401
except ImportError:
    t = types.ModuleType('tqdm')
    t.tqdm = lambda it, *a, **k: it
    t.trange = lambda *a, **k: range(*a)
    sys.modules['tqdm'] = t
import numpy as np
np.int = int
np.float = float
spec = importlib.util.spec_from_file_location('golden_inputs', sys.argv[1])
gi = importlib.util.module_from_spec(spec); spec.loader.exec_module(gi)
OUT = sys.argv[2]

from hamiltonian.models.cpu.softmax import softmax as ref_softmax
from hamiltonian.models.cpu.logistic import logistic as ref_logistic
from hamiltonian.models.cpu.mvn_gaussian import mvn_gaussian as ref_mvn
from hamiltonian.inference.cpu.metropolis import MH as ref_MH


def run(model, X, y, start, scale, seq, burnin, niter, mvn=False):
    calls = []
    if mvn:
        def logp(X_, y_, q, hyper):
            v = -model.negative_log_posterior(q)
            calls.append(float(v)); return v
    else:
        def logp(X_, y_, q, hyper):
            v = model.log_likelihood(q, X_train=X_, y_train=y_) + model.log_prior(q)
            calls.append(float(v)); return v
    mh = ref_MH(X, y, logp, start, model.hyper, scale=scale, update_sequential=seq, verbose=True)
    np.random.seed(0)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()), \
            np.errstate(over='ignore', invalid='ignore'):
        post = mh.sample(niter, burnin, np.random.RandomState(0))
    n = burnin + niter
    lp = np.array(calls).reshape(n, 2)                   # (proposal, current) per step
    with np.errstate(over='ignore', invalid='ignore'):
        A = np.exp((-lp[:, 1]) - (-lp[:, 0]))
    u = np.random.RandomState(0).rand(n)
    acc = np.isfinite(A) & (u < A)
    # the kept state's logp after a step is the next step's current-state logp
    kept = np.where(acc, lp[:, 0], lp[:, 1])
    assert np.array_equal(kept[:-1], lp[1:, 1])
    flat = np.concatenate([post[v] for v in start], axis=1)
    prev = np.concatenate([np.reshape(start[v], -1) for v in start]) if burnin == 0 else None
    for i in range(niter):
        if prev is not None:
            assert bool(np.any(flat[i] != prev)) == bool(acc[burnin + i]), i
        prev = flat[i]
    o = {'A': A, 'u': u, 'accepted': acc, 'logp': kept, 'scale': np.float64(mh._scale),
         'lines': np.array(buf.getvalue().splitlines())}
    for v in start:
        o['post_' + v] = post[v]
    return o


def save(name, groups):
    flat = {}
    for g, o in groups.items():
        for k, v in o.items():
            flat[g + '_' + k] = v
    np.savez(OUT + '/' + name, **flat)
    for g, o in groups.items():
        print(name, g, 'accept rate %.3f' % o['accepted'].mean(), 'scale', float(o['scale']),
              'min|A-u| %.2e' % np.min(np.abs(o['A'] - o['u'])[np.isfinite(o['A'])]),
              'nonfinite', int(np.sum(~np.isfinite(o['A']))))


X, Y = gi.dataset(3, 60, 24, 10)
start = {'weights': np.zeros((24, 10)), 'bias': np.zeros(10)}
m = ref_softmax({'alpha': 0.01})
save('mh_softmax.npz', {'seq': run(m, X, Y, start, 0.1, True, 8, 12),
                        'site': run(m, X, Y, start, 0.5, False, 8, 12)})

X, y, _, _ = gi.logistic_inputs(3, 77, 33)
start = {'weights': np.zeros((33, 1)), 'bias': np.zeros(1)}
m = ref_logistic({'alpha': 0.25})
save('mh_logistic.npz', {'seq': run(m, X, y, start, 0.05, True, 8, 12)})

hyper = {'mu': np.zeros(2), 'cov': np.array([[1.0, 0.8], [0.8, 1.0]])}
m = ref_mvn(hyper)
save('mh_mvn.npz', {'near': run(m, None, None, {'x': np.zeros(2)}, 1.0, True, 50, 200, mvn=True),
                    'far': run(m, None, None, {'x': np.array([60.0, -60.0])}, 30.0, True, 0, 40, mvn=True)})
print('ok')
'''


def main():
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1', OPENBLAS_NUM_THREADS='1')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'oracle', 'inputs.py'), OUT, REFERENCE],
                       env=env, capture_output=True, text=True)
    sys.stdout.write(r.stdout[-4000:])
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(r.returncode)
    info = {'generator': 'tools/gen_golden_mh.py',
            'reference': 'hamiltonian/inference/cpu/metropolis.py (class MH) with the reference CPU models',
            'files': ['mh_softmax.npz', 'mh_logistic.npz', 'mh_mvn.npz'],
            'numpy': __import__('numpy').__version__, 'OPENBLAS_NUM_THREADS': 1,
            'np_seed': 0, 'rng': 'RandomState(0)'}
    with open(os.path.join(OUT, 'PROVENANCE_mh.json'), 'w') as f:
        json.dump(info, f, indent=1)


if __name__ == '__main__':
    main()
