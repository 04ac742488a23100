"""The single-wavefront (LONE) rollout variants at batches where SIMDs hold a SECOND wave.  The rest of the suite runs them at
a few dozen environments, one wave per SIMD at the most; here 1 366 wavefronts meet 1 024 SIMDs, as in the headline launch.
A fused launch must equal its single steps bit for bit, and two fused launches must equal one.

What this does and does not pin: the plain 20 x 10 variant hands the issue priority from the younger to the older wave of a
shared SIMD part of the way through a launch (`kAgeBalance`), and only at such a batch does that path
execute.  Priority decides which wave issues, never what it computes, so these assertions cannot fail through the priority
logic as such and they hold without it too (the 10 x 10 and 5 x 3 variants do not have it).  They would fail if an edit
around that switch disturbed the step loop it sits in -- the step count, the table-copy parity, the state a launch leaves
for the next -- in a launch whose waves share SIMDs."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uavtrack():
    import uavtrack
    return uavtrack


# (N, M, B): 1 366 wavefronts of 3 / 6 / 12 environments, the last one partly filled -- a third more than an MI355X has SIMDs
@pytest.mark.parametrize("N,M,B", [(20, 10, 4096), (10, 10, 8192), (5, 3, 16384)])
def test_second_waves_of_a_simd_compute_what_first_waves_do(uavtrack, N, M, B):
    T = 10                                                  # (20 x 10: the priority changes hands before step 6)
    cfg = uavtrack.EnvConfig(n_envs=B, n_uav=N, m_targets=M, horizon=7, x_max=600.0, y_max=500.0)
    a, b, c = (uavtrack.BatchedUavEnv(cfg) for _ in range(3))
    for env in (a, b, c):
        env.reset(seed=3)
    act = torch.randint(0, 12, (T, B, N), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    many = a.step_many(act)
    assert a.variant_info()[-1] == 1, a.variant_info()      # the single-wavefront variant ran ...
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert a.kernel_info()["workgroups"] > simds            # ... on more wavefronts than there are SIMDs
    for t in range(T):                                      # T = 1 launches (20 x 10: favoured for no step at all)
        obs, rew, done = b.step(act[t])
        assert torch.equal(obs, many["obs"][t]) and torch.equal(rew, many["reward"][t]), t
        assert torch.equal(b.info["terms"], many["terms"][t]), t
        assert torch.equal(b.info["covered"], many["covered"][t]), t
        assert torch.equal(done, many["done"][t].bool()), t
    first = {k: v.clone() for k, v in c.step_many(act[:5]).items()}     # 5 + 5 steps (20 x 10: the hand-over falls elsewhere)
    second = c.step_many(act[5:])
    for k in ("obs", "reward", "terms", "covered", "done"):
        assert torch.equal(torch.cat([first[k], second[k]]), many[k]), k
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sc[k]), k
