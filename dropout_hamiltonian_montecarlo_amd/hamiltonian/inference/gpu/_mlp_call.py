"""What the callers of the dropout MLP's device entry points (sgd, sgld, sghmc, hmc_multicore) share: the
resolution of the ``masks`` argument and ``mask_provider`` into a mask mode with host buffers, the six parameter
pointers of an argument block, negative_log_posterior from an evaluation's device outputs, and the context a call
uses (``mlp_context``: the model's device context with the model's dropout ratio set, models/gpu/mlp.py's helper —
every sampler call that reaches an hmcx_mlp_* entry takes its context from it).  Nothing else here touches a device:
the callers upload what ``mask_plan`` returns.  A provider's masks are used as given: under a model whose dropout
ratio is not the default they should carry 1/(1 − dropout) where they keep."""
import numpy as np

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd._native import HmcxError

from ...models.gpu.mlp import MLP_PARAM_NAMES, mlp_context  # noqa: F401  (mlp_context: the callers' context)


def masks_off(masks_arg):
    """True for ``masks='off'``, False for None; anything else is an error."""
    if masks_arg is not None and masks_arg != 'off':
        raise ValueError("masks must be None or 'off' (inject masks through mask_provider)")
    return masks_arg == 'off'


def mask_plan(masks_arg, provider, global_step, n_fwd, B, n_mid, who):
    """The masks of a call whose step s runs n_fwd[s] forwards (the gradient forward, then its evaluations).
    Returns (mode, host_masks, mask_off, eval_off): ``masks='off'`` none; a provider — called as
    provider(global_step + s, n_fwd[s]) in step order, each answer [n_fwd[s], 3, B, n_mid] — FIXED, the answers
    concatenated in host_masks, step s's gradient forward at mask_off[s], its evaluations at eval_off[s, 0:2];
    otherwise Philox.  host_masks is None unless the provider returned some."""
    n_steps = len(n_fwd)
    mask_off, eval_off = np.zeros(n_steps, dtype=np.int64), np.zeros((n_steps, 2), dtype=np.int64)
    if masks_off(masks_arg):
        return nat.MLP_MASKS_NONE, None, mask_off, eval_off
    if provider is None:
        return nat.MLP_MASKS_PHILOX, None, mask_off, eval_off
    n3, chunks, off = 3 * B * n_mid, [], 0
    for s in range(n_steps):
        nf = int(n_fwd[s])
        mk = np.asarray(provider(global_step + s, nf))
        if mk.shape != (nf, 3, B, n_mid):
            raise HmcxError("%s: mask_provider must return [%d, 3, %d, %d]" % (who, nf, B, n_mid))
        chunks.append(mk.reshape(-1))
        mask_off[s], eval_off[s, 0], eval_off[s, 1] = off, off + n3, off + 2 * n3
        off += nf * n3
    return nat.MLP_MASKS_FIXED, np.concatenate(chunks) if chunks else None, mask_off, eval_off


def fill_params(struct_field, tensors):
    """The six device pointers of an hmcx_mlp_params field; tensors: {name: tensor} or six in canonical order."""
    if hasattr(tensors, 'keys'):
        tensors = [tensors[k] for k in MLP_PARAM_NAMES]
    for i, t in enumerate(tensors):
        struct_field.p[i] = t.data_ptr()


def nlp_from_eval(model, keys, loss, sumsq):
    """negative_log_posterior from the device's pieces, loss [...] and Σθ² per canonical variable [..., 6]:
    mlp.nlp_from_parts' float64 operations with the variables in the order of keys (the start order)."""
    sumsq = np.asarray(sumsq, dtype=np.float64)
    K = np.zeros(np.shape(loss))
    for k in keys:
        K -= 0.5 * model.alpha * sumsq[..., MLP_PARAM_NAMES.index(k)] / int(np.prod(model.shapes[k]))
    return np.asarray(loss, dtype=np.float64) + K
