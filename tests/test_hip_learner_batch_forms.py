"""The contract the ten batch entry points of the learner share (uavtrack_learner_update, _update_weighted,
_update_discounted, _update_clipped, _update_stored and the five _grad forms), called through ctypes: every host-side refusal
returns non-zero with its whole message, in one order for all ten (of two faults the earlier one's message), and leaves the
parameters, the Adam moments and step counts, theta-, the priorities and the caller's outputs byte for byte as they were,
with nothing counted by uavtrack_learner_check; the good call lands; and the forms nest: null optional pointers give the
bits of the shorter form.

H = 8, A = 12, a store of 7 slots, n = 5 rows through indices with a repeated slot, learners reserved for 16 rows: one
per_sample (target critic on) and one reference learner (which cannot arm a batch advantage and refuses the clipped and
the stored forms, so those have no good call there).  The _stored pair runs twice, with log_mu and with log_mu null
("_no_log_mu": clip_eps is then not read, so that call carries clip_eps = NaN throughout)."""
import ctypes as C

import numpy as np
import pytest
import torch

import learner_harness as lh

pytestmark = pytest.mark.gpu

DEV = lh.DEV
H, A, CAP, N, MAX_BATCH = 8, 12, 7, 5, 16
IDX = (3, 0, 6, 3, 5)                           # slot 3 twice: the later row's |delta| is its priority
KINDS = ("update", "grad")
SUFFIXES = ("", "_weighted", "_discounted", "_clipped")
FORMS = tuple(k + s for k in KINDS for s in SUFFIXES) + \
    tuple(k + s for k in KINDS for s in ("_stored", "_stored_no_log_mu"))
SENTINEL = 7.5

STORES_NULL = "states, actions, rewards and next_states must not be null"
REFERENCE = ("the clipped surrogate on a UAVTRACK_LOSS_REFERENCE learner: that form scales the actor's gradient sums once "
             "by -mean(delta) / N, a factor a per-row gate cannot share; use UAVTRACK_LOSS_PER_SAMPLE")
STORED_REFERENCE = ("stored advantages on a UAVTRACK_LOSS_REFERENCE learner: that form scales the actor's gradient sums "
                    "once by -mean(delta) / N, a factor a per-row advantage cannot share; use UAVTRACK_LOSS_PER_SAMPLE")
ADVANTAGE = ("n = 1 row under UAVTRACK_ADVANTAGE_BATCH: the standard deviation of a batch needs n >= 2 "
             "(uavtrack_learner_set_advantage)")
ENTROPY = "n = 5 rows, the installed entropy buffer holds 4 (uavtrack_learner_set_diagnostics)"
RESERVED = "n = 17 rows, scratch is reserved for 16 (uavtrack_learner_reserve)"


@pytest.fixture(scope="module")
def world():
    """The blob and the store, shared and never written."""
    rng = np.random.RandomState(11)
    s, a, r, s2 = lh.batch(rng, CAP, A)
    w = {"blob": lh.init_blob(H, A, 4),
         "store": {"states": lh.dev(s), "actions": lh.dev(a), "rewards": lh.dev(r), "next_states": lh.dev(s2)},
         "indices": lh.dev(np.array(IDX, np.int64)),
         "weights": lh.dev(rng.uniform(0.25, 1.0, size=N).astype(np.float32)),
         "discounts": lh.dev(rng.uniform(0.5, 0.95, size=CAP).astype(np.float32)),
         "log_mu": lh.dev(rng.uniform(-3.0, -1.0, size=CAP).astype(np.float32)),
         "advantages": lh.dev(rng.uniform(-1.0, 1.0, size=CAP).astype(np.float32))}
    torch.cuda.synchronize()
    return w


def _learner(world, loss):
    L = lh.learner(H, A, loss, world["blob"], max_batch=MAX_BATCH)
    if loss == "per_sample":
        L.set_target(tau=0.5)
    return L


def _outputs(L):
    """The caller's outputs of every form and a priority store, all holding a sentinel."""
    out = {k: torch.full((m,), SENTINEL, device=DEV)
           for k, m in (("actor_loss", 1), ("critic_loss", 1), ("td_delta", MAX_BATCH + 1), ("ratio_out", MAX_BATCH + 1),
                        ("priorities", CAP), ("row", L.row_floats))}
    torch.cuda.synchronize()
    return out


def _base(world, out):
    """The good call's arguments by name: addresses, sizes, scalars."""
    a = {k: v.data_ptr() for k, v in world["store"].items()}
    a.update({k: world[k].data_ptr() for k in ("indices", "weights", "discounts", "log_mu", "advantages")})
    a.update({k: v.data_ptr() for k, v in out.items()})
    a.update(n=N, capacity=CAP, clip_eps=0.2)
    return a


def _call(L, form, handle, a):
    """One direct library call; returns (rc, message)."""
    form = form.replace("_no_log_mu", "")
    kind, suffix = form.split("_")[0], form[form.index("_"):] if "_" in form else ""
    args = [a["n"], a["states"], a["actions"], a["rewards"], a["next_states"], a["capacity"], a["indices"]]
    if suffix:
        args.append(a["weights"])
    if suffix in ("_discounted", "_clipped", "_stored"):
        args.append(a["discounts"])
    if suffix == "_stored":
        args.append(a["advantages"])
    if suffix in ("_clipped", "_stored"):
        args += [a["log_mu"], a["clip_eps"], a["ratio_out"]]
    args += [a["actor_loss"], a["critic_loss"], a["td_delta"], a["priorities"]] if kind == "update" else [a["td_delta"], a["row"]]
    rc = getattr(L._lib, "uavtrack_learner_" + form)(handle, *args, L._stream())
    return rc, L._lib.uavtrack_last_error().decode()


def _image(L, out):
    """Everything a refusal must leave alone, as bytes (a NaN compares equal to itself)."""
    torch.cuda.synchronize()
    parts = [L._get_params(), *L._optim_state()] + ([L._get_target_params()] if L._target_on() else [])
    return [np.ascontiguousarray(p).tobytes() for p in parts] + [t.cpu().numpy().tobytes() for t in out.values()]


def _refused_count(L):
    refused = C.c_int64(-1)
    rc = L._lib.uavtrack_learner_check(L._h, C.byref(refused), L._stream())
    return rc, refused.value


def _faults(form, loss):
    """(label, arguments to change, setting to arm or None, the message behind the entry point's name), in the order the
    library tests them; then the pairs of two faults at once, whose message is the earlier one's.  Every text is the
    library's, written out."""
    update, clipped, per_sample = form.startswith("update"), form.endswith("_clipped"), loss == "per_sample"
    stored, log_mu = "_stored" in form, form.endswith(("_clipped", "_stored"))
    out = [(f"{k} null", {k: None}, None, STORES_NULL) for k in lh.STORES]
    outs, outs_null = (("actor_loss", "critic_loss"), "actor_loss and critic_loss must not be null") if update else \
        (("td_delta", "row"), "td_delta and row must not be null")
    out += [(f"{k} null", {k: None}, None, outs_null) for k in outs]
    out += [("n = 0", {"n": 0}, None, "n = 0 < 1"),
            ("n = -3", {"n": -3}, None, "n = -3 < 1"),
            ("n = 17", {"n": 17}, None, RESERVED),
            ("capacity = 0", {"capacity": 0}, None, "capacity = 0 < 1"),
            ("no indices, capacity 4", {"indices": None, "capacity": 4}, None, "n = 5 rows without indices from a store of 4"),
            ("entropy buffer of 4", {}, "entropy", ENTROPY)]
    if per_sample:
        out.append(("n = 1, batch advantage", {"n": 1}, "advantage", ADVANTAGE))
    if stored:
        out.append(("advantages null", {"advantages": None}, None, "advantages must not be null"))
        if not per_sample:
            out.append(("reference learner", {}, None, STORED_REFERENCE))
    if clipped:
        out.append(("log_mu null", {"log_mu": None}, None, "log_mu must not be null"))
    if log_mu and (per_sample or clipped):                                  # (_stored on a reference learner never gets here)
        out += [("clip_eps = -1", {"clip_eps": -1.0}, None, "clip_eps = -1 must be >= 0 (+inf: never clips)"),
                ("clip_eps = nan", {"clip_eps": float("nan")}, None, "clip_eps = nan must be >= 0 (+inf: never clips)")]
    if clipped and not per_sample:
        out.append(("reference learner", {}, None, REFERENCE))
    # two at once, adjacent in the order wherever one call can hold both (the null handle's pair is the caller's)
    pairs = [("stores + outputs", {"rewards": None, outs[0]: None}, None, STORES_NULL),
             ("outputs + n = 0", {outs[1]: None, "n": 0}, None, outs_null),
             ("n = 0 + capacity = 0", {"n": 0, "capacity": 0}, None, "n = 0 < 1"),
             ("n = 17 + capacity = 0", {"n": 17, "capacity": 0}, None, RESERVED),
             ("capacity = 0 + no indices", {"capacity": 0, "indices": None}, None, "capacity = 0 < 1"),
             ("no indices + entropy buffer", {"indices": None, "capacity": 4}, "entropy",
              "n = 5 rows without indices from a store of 4")]
    if clipped:
        pairs += [("entropy buffer + log_mu null", {"log_mu": None}, "entropy", ENTROPY),
                  ("log_mu null + clip_eps = -1", {"log_mu": None, "clip_eps": -1.0}, None, "log_mu must not be null")]
        if per_sample:
            pairs.append(("batch advantage + log_mu null", {"n": 1, "log_mu": None}, "advantage", ADVANTAGE))
        else:
            pairs.append(("clip_eps = -1 + reference learner", {"clip_eps": -1.0}, None,
                          "clip_eps = -1 must be >= 0 (+inf: never clips)"))
    if stored:
        pairs.append(("entropy buffer + advantages null", {"advantages": None}, "entropy", ENTROPY))
        if per_sample:
            pairs.append(("batch advantage + advantages null", {"n": 1, "advantages": None}, "advantage", ADVANTAGE))
        else:
            pairs += [("advantages null + reference learner", {"advantages": None}, None, "advantages must not be null"),
                      ("reference learner + clip_eps = -1", {"clip_eps": -1.0}, None, STORED_REFERENCE)]
        if log_mu:
            pairs.append(("advantages null + clip_eps = -1", {"advantages": None, "clip_eps": -1.0}, None,
                          "advantages must not be null"))
    return out + pairs


def _arm(L, setting, on):
    if setting == "entropy":
        L.enable_diagnostics(4) if on else L.disable_diagnostics()
    elif setting == "advantage":
        L.set_advantage("batch" if on else "raw")


@pytest.mark.parametrize("loss", ["per_sample", "reference"])
@pytest.mark.parametrize("form", FORMS)
def test_refusals_in_order_change_nothing_and_the_good_call_lands(form, loss, world):
    L = _learner(world, loss)
    fn = "uavtrack_learner_" + form.replace("_no_log_mu", "")
    out = _outputs(L)
    base = _base(world, out)
    if form.endswith("_no_log_mu"):                                         # clip_eps is read with log_mu alone
        base.update(log_mu=None, clip_eps=float("nan"))
    before = _image(L, out)

    def refused(label, handle, args, text):
        rc, msg = _call(L, form, handle, args)
        assert rc != 0, label
        assert msg == f"{fn}: {text}", label
        assert _image(L, out) == before, label
        assert _refused_count(L) == (0, 0), label

    refused("null handle", None, base, "null handle")
    refused("null handle + states null", None, dict(base, states=None), "null handle")
    for label, over, setting, text in _faults(form, loss):
        _arm(L, setting, True)
        refused(label, L._h, dict(base, **over), text)
        _arm(L, setting, False)

    if ("_clipped" in form or "_stored" in form) and loss == "reference":
        L.close()
        return
    p0, (_, _, steps0) = L._get_params(), L._optim_state()
    rc, msg = _call(L, form, L._h, base)
    assert rc == 0, msg
    assert _refused_count(L) == (0, 0)
    td = out["td_delta"].cpu().numpy()
    assert np.isfinite(td[:N]).all() and (td[N:] == SENTINEL).all()
    ratio = out["ratio_out"].cpu().numpy()
    if form.endswith(("_clipped", "_stored")):
        assert np.isfinite(ratio[:N]).all() and (ratio[N:] == SENTINEL).all()
    else:
        assert (ratio == SENTINEL).all()
    if form.startswith("update"):
        assert (L._optim_state()[2] == steps0 + 1).all() and not np.array_equal(L._get_params(), p0)
        assert np.isfinite(out["actor_loss"].item()) and np.isfinite(out["critic_loss"].item())
        prio, want = out["priorities"].cpu().numpy(), np.full(CAP, SENTINEL, np.float32)
        for row, slot in enumerate(IDX):                                    # the last occurrence of a slot wins
            want[slot] = abs(td[row])
        assert prio.tobytes() == want.tobytes()
    else:
        tail = out["row"].cpu().numpy().view(np.int32)[-4:]
        assert tail.tolist() == [N, 0, 0, L.num_params]                     # n (two words), no status bit, the layout
        assert np.array_equal(L._get_params(), p0) and (out["priorities"] == SENTINEL).all()
    L.close()


@pytest.mark.parametrize("kind", KINDS)
def test_null_optional_pointers_give_the_bits_of_the_shorter_form(kind, world):
    """plain == _weighted(NULL); _weighted(w) == _discounted(w, NULL); and _clipped at log_mu = the actor's own
    log-probabilities (ratio 1, nothing clipped) moves the parameters as the per-sample form with the same w and d."""
    def run(suffix, **over):
        L = _learner(world, "per_sample")
        out = _outputs(L)
        args = dict(_base(world, out), **over)
        if suffix == "_clipped":
            own = L.log_probs(world["store"]["states"], world["store"]["actions"])
            args["log_mu"] = own.data_ptr()
        rc, msg = _call(L, kind + suffix, L._h, args)
        assert rc == 0, msg
        assert _refused_count(L) == (0, 0)
        torch.cuda.synchronize()
        res = dict(lh.state(L), target=L._get_target_params(), **{k: v.cpu().numpy() for k, v in out.items() if k != "ratio_out"})
        L.close()
        return res

    lh.same(run(""), run("_weighted", weights=None))
    lh.same(run("_weighted"), run("_discounted", discounts=None))
    plain, clip = run("_discounted"), run("_clipped")
    keys = ("params", "exp_avg", "exp_avg_sq", "step", "target", "td_delta") if kind == "update" else ("td_delta",)
    lh.same({k: plain[k] for k in keys}, {k: clip[k] for k in keys})
    if kind == "grad":                                                      # the gradient sums and the critic's loss sum; the
        P = plain["row"].size - 8                                           # actor's loss words hold another loss
        assert plain["row"][:P].tobytes() == clip["row"][:P].tobytes()
        assert plain["row"][P + 4:].tobytes() == clip["row"][P + 4:].tobytes()
