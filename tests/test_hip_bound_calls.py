"""The rollout call path from both ends: the bound callables (bind_step_many, bind_run) against the eager methods they
share their argument builder with, and every refusal of the nine stepping entry points straight through the C ABI.

Shapes: 9 x 5 x 3 (the last workgroup is partly filled), T = 7 for the bound calls and T = 3 for the refusals, which
launch nothing.  Every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N, M, T = 9, 5, 3, 7
SEED = 11


def make_env(mode, actor=True, pmi_sd=None, **kw):
    import uavtrack
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, cooperative=0.0 if mode == "RAW" else 0.3,
                             reward_mode=getattr(uavtrack.RewardMode, mode), **kw)
    env = uavtrack.BatchedUavEnv(cfg, DEV)
    if pmi_sd is not None:
        env.set_pmi(pmi_sd)
    if actor:
        torch.manual_seed(5)
        net = uavtrack.ActorMLP(hidden_dim=32, action_dim=cfg.na_total)
        with torch.no_grad():
            net.fc2.weight.mul_(5.0)      # (probabilities away from uniform)
        env.set_actor(net)
    return env


# ---- bound calls == eager calls ------------------------------------------------------------------------------------------
def _bound_out(with_actions):
    out = dict(obs=torch.empty(T, B, N, 12, device=DEV), reward=torch.empty(T, B, N, device=DEV),
               terms=torch.empty(T, 3, B, N, device=DEV), covered=torch.empty(T, B, dtype=torch.int32, device=DEV),
               done=torch.empty(T, B, dtype=torch.uint8, device=DEV), ep_sums=torch.empty(B, 5, device=DEV))
    if with_actions:
        out["actions"] = torch.empty(T, B, N, dtype=torch.int32, device=DEV)
    return out


@pytest.mark.parametrize("mode", ["RAW", "MEAN"])
def test_bound_calls_equal_eager_calls(mode):
    """bind_step_many(actions, out)() == step_many(actions); bind_run(T, out, "greedy")() == run_greedy(T);
    bind_run(T, out, "actor", mode=m)() == run_actor(T, m) for both modes: two calls each on two handles that start from
    the same state, every output and the final state; the bound call returns the `out` it was given."""
    import uavtrack
    g = torch.Generator(DEV).manual_seed(3)
    acts = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device=DEV, generator=g)
    forms = [("step_many", lambda e, o, out: e.bind_step_many(acts, out), lambda e, o: e.step_many(acts)),
             ("greedy", lambda e, o, out: e.bind_run(T, out, "greedy", seed=SEED), lambda e, o: e.run_greedy(T, seed=SEED))]
    for m in (uavtrack._lib.ACTOR_SAMPLE, uavtrack._lib.ACTOR_ARGMAX):
        forms.append((f"actor-{m}", lambda e, o, out, m=m: e.bind_run(T, out, "actor", obs_in=o, seed=SEED, mode=m),
                      lambda e, o, m=m: e.run_actor(T, o, seed=SEED, mode=m)))
    for name, bind, eager in forms:
        a, b = make_env(mode), make_env(mode)
        oa, ob = a.reset(seed=2), b.reset(seed=2)
        assert torch.equal(oa, ob)
        out = _bound_out(name != "step_many")
        call = bind(a, oa, out)
        for k in range(2):
            assert call() is out, name
            want = eager(b, ob)
            assert set(out) == set(want), (name, sorted(out), sorted(want))
            for key in out:
                assert torch.equal(out[key], want[key]), (mode, name, k, key)
        sa, sb = a.get_state(), b.get_state()
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (mode, name, key)
        a.close(); b.close()


# ---- refusals, straight through the C ABI ----------------------------------------------------------------------------
TR = 3
OUTS = ("obs", "reward", "terms", "covered", "done")
ENTRIES = {
    "uavtrack_step": ("h", "actions") + OUTS + ("stream",),
    "uavtrack_step_accumulate": ("h", "actions") + OUTS + ("ep_sums", "stream"),
    "uavtrack_step_many": ("h", "T", "actions") + OUTS + ("ep_sums", "stream"),
    "uavtrack_step_many_autoreset": ("h", "T", "reset_seed", "actions") + OUTS + ("ep_sums", "stream"),
    "uavtrack_run_greedy": ("h", "T", "seed", "actions_out") + OUTS + ("ep_sums", "stream"),
    "uavtrack_run_greedy_autoreset": ("h", "T", "seed", "reset_seed", "actions_out") + OUTS + ("ep_sums", "stream"),
    "uavtrack_run_actor": ("h", "T", "seed", "mode", "obs_in", "actions_out") + OUTS + ("ep_sums", "stream"),
    "uavtrack_run_actor_autoreset": ("h", "T", "seed", "reset_seed", "mode", "obs_in", "actions_out") + OUTS + ("ep_sums", "stream"),
    "uavtrack_step_host": ("h", "actions_host", "host_out", "stream"),
}
ALL = tuple(ENTRIES)
DEVICE = ALL[:-1]                                  # every entry but uavtrack_step_host
WITH_T = ALL[2:-1]
AUTORESET = tuple(e for e in ALL if e.endswith("_autoreset"))
GREEDY = tuple(e for e in ALL if "greedy" in e)
ACTOR = tuple(e for e in ALL if "actor" in e)
GIVEN = ALL[:4]
INSTALL = {"tpos": "uavtrack_set_target_trace", "raw": "uavtrack_set_raw_reward_output", "start_obs": "uavtrack_set_start_obs_output"}

# (the one thing wrong, the handle it is tried on, the entry points it applies to, what the message says): one row per
# check of the acceptance order -- null handle; the combination without a kernel; no horizon; T; actions; reward; the
# actor's four; the three capacities; MAAC-R without weights -- and uavtrack_step_accumulate's own ep_sums
ROWS = [
    (dict(h=None), "plain", ALL, "null handle"),
    ({}, "dim3", GREEDY, "planar"),
    ({}, "pmi", GREEDY, "MAAC / MAAC-G"),
    ({}, "nohorizon", AUTORESET, "no horizon"),
    (dict(T=0), "plain", WITH_T, "T must be >= 1 (got 0)"),
    (dict(actions=None), "plain", GIVEN, "actions is null"),
    (dict(reward=None), "plain", DEVICE, "reward is null"),
    (dict(obs_in=None), "plain", ACTOR, "obs_in is null"),
    ({}, "noactor", ACTOR, "needs uavtrack_set_actor_weights first"),
    (dict(mode=7), "plain", ACTOR, "mode 7 is neither UAVTRACK_ACTOR_SAMPLE nor UAVTRACK_ACTOR_ARGMAX"),
    (dict(obs_in="obs"), "plain", ACTOR, "obs_in must not alias obs when T > 1"),
    (dict(install="tpos"), "plain", WITH_T, "T = 3 exceeds the 2 steps the target-trace buffer holds"),
    (dict(install="raw"), "plain", WITH_T, "T = 3 exceeds the 2 steps the raw-reward buffer holds"),
    (dict(install="start_obs"), "plain", AUTORESET, "T = 3 exceeds the 2 steps the start-observation buffer holds"),
    ({}, "pmi_noweights", tuple(e for e in ALL if e not in GREEDY), "reward_mode PMI needs uavtrack_set_pmi_weights first"),
    (dict(ep_sums=None), "plain", ("uavtrack_step_accumulate",), "ep_sums is null"),
]


def test_refusals_through_the_c_abi(pmi_state_dict):
    """Every refusal of the stepping entry points, each with exactly one thing wrong: a non-zero return code, the
    message with its text and the entry point's name, the state and the sentinel-filled outputs untouched."""
    SENT = -7
    envs = dict(plain=make_env("RAW", horizon=4), nohorizon=make_env("RAW", horizon=0), noactor=make_env("RAW", actor=False, horizon=4),
                dim3=make_env("RAW", actor=False, horizon=4, dim=3, nc=3), pmi=make_env("PMI", actor=False, pmi_sd=pmi_state_dict, horizon=4),
                pmi_noweights=make_env("PMI", horizon=4))
    for k, e in enumerate(envs.values()):
        e.reset(seed=k)
    lib = envs["plain"]._lib
    f32 = lambda *shape: torch.full(shape, float(SENT), device=DEV)
    outs = dict(obs=f32(TR, B, N, 12), reward=f32(TR, B, N), terms=f32(TR, 3, B, N), ep_sums=f32(B, 5),
                covered=torch.full((TR, B), SENT, dtype=torch.int32, device=DEV),
                done=torch.full((TR, B), 7, dtype=torch.uint8, device=DEV),
                actions_out=torch.full((TR, B, N), SENT, dtype=torch.int32, device=DEV),
                small=f32(TR - 1, B, N, 12))               # the installed buffer of the capacity rows (large enough for any of the three)
    pristine = {k: v.clone() for k, v in outs.items()}
    given = dict(actions=torch.ones(TR, B, N, dtype=torch.int32, device=DEV), obs_in=torch.zeros(B, N, 12, device=DEV))
    host_actions = np.ones((B, N), np.int32)
    tried = 0
    for wrong, kind, entries, text in ROWS:
        env = envs[kind]
        for entry in entries:
            good = dict(h=env._h, T=TR, seed=SEED, reset_seed=5, mode=0, stream=env._stream(),
                        actions_host=C.c_void_p(host_actions.ctypes.data), host_out=C.byref(env._host_step),
                        **{k: v.data_ptr() for k, v in {**outs, **given}.items()})
            install = wrong.get("install")
            for k, v in wrong.items():
                if k != "install":
                    good[k] = good[v] if isinstance(v, str) else v
            before = env.get_state()
            if install:
                assert getattr(lib, INSTALL[install])(env._h, outs["small"].data_ptr(), TR - 1) == 0
            rc = getattr(lib, entry)(*[good[a] for a in ENTRIES[entry]])
            msg = lib.uavtrack_last_error().decode()
            if install:
                assert getattr(lib, INSTALL[install])(env._h, None, 0) == 0
            torch.cuda.synchronize()
            assert rc != 0, (entry, wrong, kind)
            assert text in msg and entry + ":" in msg, (entry, wrong, kind, msg)
            after = env.get_state()
            for k in before:
                assert torch.equal(before[k], after[k]), (entry, wrong, kind, k)
            for k in outs:
                assert torch.equal(outs[k], pristine[k]), (entry, wrong, kind, k)
            tried += 1
    assert tried == sum(len(entries) for _, _, entries, _ in ROWS)
    for e in envs.values():
        e.close()
