"""The library calls behind update_from, grad_from, update_from_many and update_from(group=) are the recorded ones:
tests/golden/learner_calls.json is the trace of tests/learner_call_trace.py's matrix (buffers x paths x options) as it
was before the options travelled as one DrawSpec and the buffers drew through _draw_batch.  No GPU: the learners and
rings carry no handle, and the library is a recorder."""
import json

import learner_call_trace as lt


def _golden():
    with open(lt.GOLDEN) as f:
        return json.load(f)


def test_every_case_of_the_matrix_is_in_the_golden():
    # 2 rings x (plain, n-step, lambda, behaviour, n-step + behaviour), the 2 torch buffers, a ring folded with another
    # gamma, an empty ring; the 4 paths; the 7 option sets
    assert len(lt.BUFFERS) == 2 * 5 + 2 + 1 + 1 and len(lt.PATHS) == 4 and len(lt.OPTIONS) == 7
    keys = lt.case_keys()
    assert len(keys) == len(set(keys)) == 14 * 4 * 7
    golden = _golden()
    assert sorted(golden) == sorted(keys)
    assert all(golden[k] for k in keys)                                     # no case without a call or an error


def test_the_calls_are_the_recorded_ones():
    golden = _golden()
    for key in lt.case_keys():
        assert lt.run_case(key) == golden[key], key


def test_draw_batch_always_returns_a_pair_and_sample_draws_through_it():
    spec = lt.uavtrack.replay.DrawSpec
    assert spec() == (False, 0.4, None, 0, None, None, None)
    assert spec._fields == ("importance", "beta", "beta_final", "anneal_calls", "rho_bar", "rho_out", "generator")
    for which in lt.BUFFERS[:-1]:
        for s in (spec(), spec(importance=True, beta=0.5)):
            lt.REC.calls, lt.REC.known, lt.REC.fresh, lt.REC.dump = [], {}, [], False
            buf = lt.make_buffer(which)
            idx, w = buf._draw_batch(4, s)
            assert idx.shape == (4,) and idx.dtype == lt.torch.int64
            assert (w is not None) == (s.importance and buf.priorities is not None)
            for attr in ("priorities", "discounts", "log_mu", "gamma"):
                assert hasattr(buf, attr)
