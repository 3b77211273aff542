"""cacto_update_plan (RL_AC.update_plan) reports the route the update calls take, and the split
weight-gradient GEMM + Adam kernels of every form (k_wgrad, k_wgrad_big, k_adam<NCH>, the looped
k_adam<0> / k_reduce<0>) give the bits of the gradient call followed by the Adam call."""
import numpy as np
import pytest
import torch

from cacto_amd.confs import load_conf
from cacto_amd.environment import make_env
from cacto_amd.neural_network import NN
from cacto_amd.rl import ACTOR, CRITIC, RL_AC

pytestmark = pytest.mark.gpu

# The route of a double-integrator batch with the sine critic, written out from the rules (Bp = B
# rounded up to 16; rows: critic 2 Bp with w_S != 0 else Bp, actor Bp):
#   chunk 64 rows up to 1024 rows, 128 below 4096, 256 from there on; nch = ceil(rows / chunk)
#   paired (gemm 0) while 2 Bp <= 1024; 4-sample tiles up to Bp = 512
#   gemm 2 (k_wgrad_big) above 1024 rows, else 1; xcd from 8 chunks on
#   xcd_tiles when Bp / 16 is a multiple of 128 and both chunks are 256
#   adam_nch the smallest of 8, 16, 32, 64 that holds nch, else 0
#   pair_xcds: the power of two (<= 8) with 2 Bp / 4 tiles <= 8 per XCD, for the 4-sample tiles
# A network's entry: (rows, chunk, nch, gemm, xcd, adam_nch). crit1: w_S = 1e-2, crit0: w_S = 0.
ROUTE = {
    1: dict(Bp=16, tile=4, paired=1, crit1=(32, 64, 1, 0, 0, 8), crit0=(16, 64, 1, 0, 0, 8),
            act=(16, 64, 1, 0, 0, 8), xcd_tiles=0, pair_xcds=1),
    16: dict(Bp=16, tile=4, paired=1, crit1=(32, 64, 1, 0, 0, 8), crit0=(16, 64, 1, 0, 0, 8),
             act=(16, 64, 1, 0, 0, 8), xcd_tiles=0, pair_xcds=1),
    17: dict(Bp=32, tile=4, paired=1, crit1=(64, 64, 1, 0, 0, 8), crit0=(32, 64, 1, 0, 0, 8),
             act=(32, 64, 1, 0, 0, 8), xcd_tiles=0, pair_xcds=2),
    512: dict(Bp=512, tile=4, paired=1, crit1=(1024, 64, 16, 0, 1, 16), crit0=(512, 64, 8, 0, 1, 8),
              act=(512, 64, 8, 0, 1, 8), xcd_tiles=0, pair_xcds=8),
    513: dict(Bp=528, tile=16, paired=0, crit1=(1056, 128, 9, 2, 1, 16), crit0=(528, 64, 9, 1, 1, 16),
              act=(528, 64, 9, 1, 1, 16), xcd_tiles=0, pair_xcds=0),
    1024: dict(Bp=1024, tile=16, paired=0, crit1=(2048, 128, 16, 2, 1, 16), crit0=(1024, 64, 16, 1, 1, 16),
               act=(1024, 64, 16, 1, 1, 16), xcd_tiles=0, pair_xcds=0),
    1025: dict(Bp=1040, tile=16, paired=0, crit1=(2080, 128, 17, 2, 1, 32), crit0=(1040, 128, 9, 2, 1, 16),
               act=(1040, 128, 9, 2, 1, 16), xcd_tiles=0, pair_xcds=0),
    2048: dict(Bp=2048, tile=16, paired=0, crit1=(4096, 256, 16, 2, 1, 16), crit0=(2048, 128, 16, 2, 1, 16),
               act=(2048, 128, 16, 2, 1, 16), xcd_tiles=0, pair_xcds=0),
    4096: dict(Bp=4096, tile=16, paired=0, crit1=(8192, 256, 32, 2, 1, 32), crit0=(4096, 256, 16, 2, 1, 16),
               act=(4096, 256, 16, 2, 1, 16), xcd_tiles=1, pair_xcds=0),
    8192: dict(Bp=8192, tile=16, paired=0, crit1=(16384, 256, 64, 2, 1, 64), crit0=(8192, 256, 32, 2, 1, 32),
               act=(8192, 256, 32, 2, 1, 32), xcd_tiles=1, pair_xcds=0),
    8193: dict(Bp=8208, tile=16, paired=0, crit1=(16416, 256, 65, 2, 1, 0), crit0=(8208, 256, 33, 2, 1, 64),
               act=(8208, 256, 33, 2, 1, 64), xcd_tiles=0, pair_xcds=0),
}
# cacto_workspace_bytes of the parent commit's build at those batches (DI; sine critic, elu critic)
WS_BYTES = {
    "sine": {1: 1307392, 16: 1307392, 17: 1477888, 512: 10264064, 513: 9880320, 1024: 17892864, 1025: 16282368,
             2048: 28808704, 4096: 52528640, 8192: 104310272, 8193: 104871168},
    "elu": {1: 2649600, 16: 2649600, 17: 2865152, 512: 15740928, 513: 14124544, 1024: 24811520, 1025: 23428608,
            2048: 38610944, 4096: 71018496, 8192: 140175360, 8193: 140963840},
}
NET = ("rows", "chunk", "nch", "gemm", "xcd", "adam_nch")


def _expected(B, sobolev, elu, cus):
    e = ROUTE[B]
    crit = list(e["crit1"] if sobolev else e["crit0"])
    tile, pair_xcds = e["tile"], e["pair_xcds"]
    if elu:  # 16-sample tiles only (so no paired q4 grid), and never k_wgrad_big: 16/32/256/256 has 1 x 1 blocks
        tile, pair_xcds = 16, 0
        crit[3] = min(crit[3], 1)
    plan = dict(Bp=e["Bp"], chain_tile=tile, elu=int(elu), paired=e["paired"], xcd_tiles=e["xcd_tiles"],
                pair_xcds=pair_xcds, cus=cus)
    plan.update({"critic_" + k: v for k, v in zip(NET, crit)})
    plan.update({"actor_" + k: v for k, v in zip(NET, e["act"])})
    # the critic on k_wgrad_big with every chunk in one k_adam<NCH>
    plan["per_overlap"] = int(crit[3] == 2 and crit[5] != 0)
    # 16-sample tiles, at most one actor workgroup per CU
    plan["devwait_actor"] = int(tile == 16 and e["Bp"] // 16 <= cus)
    return plan


@pytest.mark.parametrize("critic_type", ["sine", "elu"])
def test_update_plan_matches_route(critic_type):
    conf = load_conf("double_integrator", fresh=True)
    conf.critic_type = critic_type
    env = make_env(conf)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for w_S in (0.0, 1e-2):
        rl = RL_AC(env, NN(env, conf, w_S=w_S, seed=0), conf)
        rl.setup_model()
        for B in ROUTE:
            got, want = rl.update_plan(B), _expected(B, w_S != 0.0, critic_type == "elu", cus)
            print(critic_type, w_S, B, got)
            assert got == want, (critic_type, w_S, B, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
            assert rl.sys.workspace_bytes(B) == WS_BYTES[critic_type][B], (critic_type, B)


@pytest.mark.parametrize("B,w_S", [(513, 0.0), (513, 1e-2), (1025, 1e-2), (8193, 1e-2)])
def test_split_gemm_adam_equals_grad_then_apply(B, w_S):
    """Above the fused batches an update runs the split GEMM and k_adam on the slabs; the gradient call
    sums the same slabs (k_reduce) and cacto_adam_step applies the sum (k_adam<8> on one chunk): the same
    sums in chunk order and the same Adam arithmetic, so three updates leave the same bits.
    (513, 0): k_wgrad + k_adam<16> for both networks; (513, 1e-2): the critic on k_wgrad_big; (1025,
    1e-2): the actor's first k_wgrad_big batch; (8193, 1e-2): 65 critic chunks, the looped k_adam<0> and
    k_reduce<0>."""
    conf = load_conf("double_integrator", fresh=True)
    env = make_env(conf)
    ns = conf.nb_state
    rng = np.random.default_rng(17)
    N = 3000
    S = np.column_stack([rng.uniform(-3, 3, (N, ns - 1)), rng.uniform(0, 4.9, N)])
    rows = np.concatenate([S, rng.normal(size=(N, 1)), S + 0.01, rng.normal(size=(N, ns)) * 0.3,
                           (rng.uniform(size=(N, 1)) < 0.1).astype(float), (rng.uniform(size=(N, 1)) < 0.1)
                           .astype(float)], axis=1)
    storage = torch.as_tensor(rows, device="cuda")
    idx = torch.as_tensor(rng.integers(0, N, size=(3, B)).astype(np.int32), device="cuda")
    wts = torch.as_tensor(rng.uniform(0.2, 1.0, size=(3, B)).astype(np.float32), device="cuda")

    def learner():
        rl = RL_AC(env, NN(env, conf, w_S=w_S, seed=4), conf)
        rl.setup_model()
        return rl

    def state(rl):
        return [t.clone() for t in (rl.actor_model.buf, rl.critic_model.buf, rl.target_critic.buf, rl.actor_m,
                                    rl.actor_v, rl.critic_m, rl.critic_v, rl.steps)]
    whole, split = learner(), learner()
    for k in range(3):
        whole.update_rows(storage, idx[k], wts[k])
        gc = split.critic_grad_flat(storage, idx[k], wts[k])
        split.apply_gradients(CRITIC, gc, soft_update=not conf.MC)
        ga = split.actor_grad_flat(storage, idx[k])
        split.apply_gradients(ACTOR, ga)
    torch.cuda.synchronize()
    for a, b in zip(state(whole), state(split)):
        assert torch.equal(a, b)
    assert int(whole.steps[0]) == 3 and int(whole.steps[1]) == 3
