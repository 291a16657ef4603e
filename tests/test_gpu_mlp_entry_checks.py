"""The seven struct-taking MLP entry points on a real context: a defective argument block returns the status and
message of csrc/hmcx_mlp_checks.h (pinned row by row on the CPU in test_mlp_checks_cpu.py), launches nothing — the
state and the outputs keep their bytes — and a valid call afterwards succeeds."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N_IN, N_MID, N_OUT, C, NS = 4, 3, 8, 2, 2, 2
SENTINEL = -7.0


def test_defective_blocks_are_rejected_before_any_launch():
    import torch
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu._mlp_call import fill_params
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES, mlp_param_shapes

    ctx = nat.context("cuda:0")
    f64 = dict(dtype=torch.float64, device="cuda:0")
    shapes = mlp_param_shapes(N_IN, N_MID, N_OUT)
    rs = np.random.RandomState(5)
    X = torch.as_tensor(rs.rand(NS * B, N_IN)).to(**f64)
    y = torch.as_tensor(rs.randint(0, N_OUT, NS * B).astype(np.int32)).to("cuda:0")

    def stack(fill=None):                                      # six [C, *shape] tensors, canonical order
        return [torch.as_tensor(rs.normal(0, 0.3, (C,) + shapes[k])).to(**f64) if fill is None
                else torch.full((C,) + shapes[k], fill, **f64) for k in MLP_PARAM_NAMES]
    par, aux, aux2 = stack(), stack(0.0), stack(0.0)
    out = torch.full((64,), SENTINEL, **f64)                   # every float64 output of a call, 16 values each
    out_i = torch.full((16,), -7, dtype=torch.int32, device="cuda:0")
    row0 = np.arange(NS, dtype=np.int64) * B
    eps = np.full(NS, 1e-3)
    n_iter = np.ones(NS * C, dtype=np.int32)
    u = np.full(NS * C, 0.5)
    keep = []                                                  # host arrays a block points to

    def host(a, ct):
        keep.append(np.ascontiguousarray(a))
        return keep[-1].ctypes.data_as(ct)

    def common(a):
        a.dtype, a.n_in, a.n_mid, a.n_out = 1, N_IN, N_MID, N_OUT          # HMCX_F64
        a.X, a.y = X.data_ptr(), y.data_ptr()
        for name, val in (("B", B), ("n_steps", NS), ("alpha", 0.01), ("seed", 3)):
            if hasattr(a, name):
                setattr(a, name, val)
        if hasattr(a, "order"):
            for i in range(6):
                a.order[i] = i
        if hasattr(a, "par"):
            fill_params(a.par, par)
        return a

    def sghmc(a):
        a.row0, a.eps = host(row0, nat.c_i64p), host(eps, nat.c_dblp)
        a.n_iter, a.u_accept = host(n_iter[:NS], nat.c_i32p), host(u[:NS], nat.c_dblp)
        a.noise_mode = a.mask_mode = nat.NOISE_PHILOX
        a.out_A, a.out_loss, a.out_accepted = out[0:].data_ptr(), out[16:].data_ptr(), out_i.data_ptr()

    def leapfrog(a):
        a.n_iter, a.eps, a.mask_mode = 1, 1e-3, nat.MLP_MASKS_NONE
        fill_params(a.q, par), fill_params(a.p, aux), fill_params(a.g, aux2)

    def sgd(a):
        a.row0, a.mask_mode, a.step_size, a.gamma = host(row0, nat.c_i64p), nat.MLP_MASKS_PHILOX, 1e-3, 0.9
        fill_params(a.mom, aux)
        a.out_loss = out.data_ptr()

    def sgld(a):
        a.row0, a.eps = host(row0, nat.c_i64p), host(eps, nat.c_dblp)
        a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
        a.out_loss = out.data_ptr()

    def sgld_chains(a):
        sgld(a)
        a.C = C

    def hmc_chains(a):
        a.B, a.C, a.eps = NS * B, C, host(eps, nat.c_dblp)
        a.n_iter, a.u_accept = host(n_iter, nat.c_i32p), host(u, nat.c_dblp)
        a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
        a.out_A, a.out_E, a.out_accepted = out[0:].data_ptr(), out[16:].data_ptr(), out_i.data_ptr()

    def predictive(a):
        a.N, a.S, a.T, a.mask_mode = NS * B, C, 1, nat.MLP_MASKS_NONE
        a.out_mean = out.data_ptr()

    def bad_n_iter(a):
        a.n_iter = host(np.array([1, 1, 1, -1], dtype=np.int32), nat.c_i32p)

    def bad_row0(a):
        a.row0 = host(np.array([0, -1], dtype=np.int64), nat.c_i64p)

    def repeat_order(a):
        a.order[5] = 0
    entries = [  # (entry, block type, the valid block's fields, the defect, status, message)
        ("hmcx_mlp_sghmc_run", nat.MlpSghmcArgs, sghmc, lambda a: setattr(a, "mask_mode", 2), -1, "bad mask_mode"),
        ("hmcx_mlp_hmc_leapfrog", nat.MlpLeapfrogArgs, leapfrog, repeat_order, -1,
         "mlp leapfrog: order must be a permutation of 0..5"),
        ("hmcx_mlp_sgd_run", nat.MlpSgdArgs, sgd, bad_row0, -1, "mlp sgd: negative row0"),
        ("hmcx_mlp_sgld_run", nat.MlpSgldArgs, sgld, lambda a: setattr(a, "variant", 2), -1,
         "mlp sgld: variant must be 0 or 1"),
        ("hmcx_mlp_sgld_chains_run", nat.MlpSgldChainsArgs, sgld_chains, lambda a: setattr(a, "C", 65), -1,
         "mlp sgld chains: C must be 1 .. 64"),
        ("hmcx_mlp_hmc_chains_run", nat.MlpHmcChainsArgs, hmc_chains, bad_n_iter, -1, "mlp hmc chains: n_iter < 0"),
        ("hmcx_mlp_predictive", nat.MlpPredictiveArgs, predictive,
         lambda a: (setattr(a, "S", 70000), setattr(a, "T", 70000)), -4, "mlp predictive: too many draws"),
    ]
    for name, block, fields, defect, status, message in entries:
        before = [t.clone() for t in par + aux + aux2]
        a = common(block())
        fields(a)
        defect(a)
        rc = getattr(ctx.lib, name)(ctx.h, ctypes.byref(a))
        torch.cuda.synchronize()
        assert (rc, ctx.lib.hmcx_last_error(ctx.h).decode()) == (status, message), name
        assert bool((out == SENTINEL).all()) and bool((out_i == -7).all()), name
        assert all(torch.equal(t, t0) for t, t0 in zip(par + aux + aux2, before)), name
        a = common(block())
        fields(a)
        rc = getattr(ctx.lib, name)(ctx.h, ctypes.byref(a))
        torch.cuda.synchronize()
        assert rc == 0, (name, ctx.lib.hmcx_last_error(ctx.h).decode())
        ran = aux2[0][0, 0, 0] if name == "hmcx_mlp_hmc_leapfrog" else out[0]    # the gradient there, an output here
        assert float(ran) not in (0.0, SENTINEL) and bool(torch.isfinite(ran)), name
        out.fill_(SENTINEL)
        out_i.fill_(-7)
