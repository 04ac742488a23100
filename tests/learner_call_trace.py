"""The library calls the learner's four drawn-update paths enqueue, written down without a GPU: handle-less learners and
rings on CPU tensors whose `_lib` is a recorder (every uavtrack_* call appends its name and arguments and returns 0), over
a matrix of buffers x paths x options.  tests/golden/learner_calls.json holds the trace as it was recorded
(`python tests/learner_call_trace.py --record`) before DrawSpec and the buffers' _draw_batch existed;
tests/test_learner_calls_cpu.py asserts that today's trace is that one.  `--time` prints the host-side cost of update_from
and of update_from_many over eight rings against the same recorder.

An argument is written as None, a scalar's value, "ringstruct" (the by-reference struct uavtrack_replay_ring), the known
tensor it points into with the element offset ("ring0._idx+0", "ring1.priorities+0", "rho_out0+0"), or "fresh<k>": the
k-th address of the case that belongs to no known tensor, i.e. to one the call allocated itself.  A case that raises ends
with the exception's type and message.  For the two torch buffers a case also records what was drawn: the indices, the
weights as float32 bit patterns and a digest of the generator's state after the call, then the same from an equally
seeded sample()."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "marl-uavs-targets-tracking_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import uavtrack                                                       # noqa: E402
from uavtrack import sharding                                         # noqa: E402
from uavtrack.learner import row_floats                               # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "learner_calls.json")
CPU = torch.device("cpu")
H, A, GAMMA, BATCH = 8, 12, 0.95, 8


class Recorder:
    """Stands in for the loaded library: uavtrack_<anything>(*args) is written down and succeeds."""

    def __init__(self):
        self.calls, self.known, self.fresh, self.dump = [], {}, [], False

    def __getattr__(self, name):
        if not name.startswith("uavtrack_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(f"{name}({', '.join(self._arg(a) for a in args)})")
            if self.dump and name.startswith(("uavtrack_learner_update", "uavtrack_learner_grad")):
                self._dump_draw(name, args)
            return 0
        return call

    def _arg(self, a) -> str:
        if a is None or isinstance(a, (bool, int, float, str)):
            return repr(a) if isinstance(a, float) else str(a)
        if isinstance(a, C.c_void_p):
            return self._address(a.value)
        if type(a).__name__ == "CArgObject":
            return "ringstruct"
        raise TypeError(f"an argument the trace has no notation for: {a!r}")

    def _address(self, addr) -> str:
        if addr is None:
            return "None"
        for name, t in self.known.items():
            lo = t.data_ptr()
            if lo <= addr < lo + max(1, t.numel()) * t.element_size():
                return f"{name}+{(addr - lo) // t.element_size()}"
        if addr not in self.fresh:
            self.fresh.append(addr)
        return f"fresh{self.fresh.index(addr)}"

    def _dump_draw(self, name, args):
        """The indices (int64) and weights (float32 bits) a torch buffer's draw handed to an update or grad call."""
        n, idx = args[1], args[7]
        weighted = name.endswith(("_weighted", "_discounted"))
        w = args[8] if weighted else None
        self.calls.append("  drew " + json.dumps(list((C.c_int64 * n).from_address(idx.value))))
        if w is not None and w.value is not None:
            self.calls.append("  weights " + json.dumps(list((C.c_uint32 * n).from_address(w.value))))


REC = Recorder()


class Learner(uavtrack.DeviceActorCritic):
    """The host-side state of a learner without its device handle."""

    def __init__(self, gamma=GAMMA):
        self.device, self.hidden_dim, self.action_dim, self.gamma, self.loss = CPU, H, A, float(gamma), "per_sample"
        self.row_floats = row_floats(H, A)
        self._lib, self._h = REC, "learner"

    def _stream(self):
        return None

    def close(self):                                                  # no handle: nothing to destroy (or to record)
        pass


def _bare_ring(cls, name, capacity, count, max_batch=16):
    class Bare(cls):
        def __init__(self):
            self.capacity, self.device, self.seed, self.max_batch = capacity, CPU, 0, max_batch
            self.store = {"states": torch.zeros(capacity, 12), "actions": torch.zeros(capacity, dtype=torch.int32),
                          "rewards": torch.arange(capacity, dtype=torch.float32), "next_states": torch.zeros(capacity, 12)}
            self.pos, self.count = count % capacity, count
            self._idx = torch.zeros(max_batch, dtype=torch.int64)
            self._lib, self._h = REC, name + ".h"
            if issubclass(cls, uavtrack.PrioritizedReplayRing):
                self.alpha = 0.6
                self.priorities = torch.ones(capacity)
                self._w = torch.zeros(max_batch)

        def _stream(self):
            return None

        def close(self):
            pass

    Bare.__name__ = cls.__name__
    return Bare()


def _torch_buffer(cls, capacity, count):
    buf = cls(capacity, "cpu")
    rng = np.random.RandomState(capacity)
    buf.add({"states": torch.zeros(count, 12), "actions": torch.zeros(count, dtype=torch.int32),
             "rewards": torch.arange(count, dtype=torch.float32), "next_states": torch.zeros(count, 12)})
    if hasattr(buf, "priorities") and buf.priorities is not None:
        buf.priorities[:count] = torch.from_numpy(rng.uniform(0.1, 2.0, count).astype(np.float32))
    return buf


RING_FORMS = {
    "plain": lambda r: r,
    "nstep": lambda r: r.with_nstep(3, 0.95),
    "lambda": lambda r: r.with_lambda(0.9, 0.95),
    "behaviour": lambda r: r.with_behaviour(),
    "nstep+behaviour": lambda r: r.with_nstep(3, 0.95).with_behaviour(),
}
BUFFERS = [f"{cls}.{form}" for cls in ("ReplayRing", "PrioritizedReplayRing") for form in RING_FORMS] + [
    "DeviceReplayBuffer", "PrioritizedDeviceReplayBuffer", "PrioritizedReplayRing.other_gamma", "ReplayRing.empty"]
PATHS = ["update_from", "grad_from", "update_from_many", "update_from_group"]
OPTIONS = {
    "defaults": {},
    "importance": dict(importance=True),
    "annealed": dict(importance=True, beta=0.7, beta_final=1.0, anneal_calls=10),
    "rho_bar": dict(rho_bar=1.0),
    "rho_bar+rho_out": dict(rho_bar=2.0, rho_out=True),
    "importance+rho_bar": dict(importance=True, rho_bar=1.0),
    "rho_out_alone": dict(rho_out=True),
}


def case_keys():
    return [f"{b}|{p}|{o}" for b in BUFFERS for p in PATHS for o in OPTIONS]


def make_buffer(which: str, name: str = "ring0"):
    if which in ("DeviceReplayBuffer", "PrioritizedDeviceReplayBuffer"):
        return _torch_buffer(getattr(uavtrack, which), 32, 20)
    cls, form = which.split(".")
    if form == "empty":
        return _bare_ring(getattr(uavtrack, cls), name, 32, 0)
    if form == "other_gamma":
        return _bare_ring(getattr(uavtrack, cls), name, 32, 20).with_nstep(3, 0.9).with_behaviour()
    return RING_FORMS[form](_bare_ring(getattr(uavtrack, cls), name, 32, 20))


def make_partner(which: str):
    """update_from_many's second buffer: of the other kind, smaller than the batch."""
    if which.startswith("Prioritized"):
        return _bare_ring(uavtrack.ReplayRing, "ring1", 24, 5).with_nstep(3, 0.95).with_behaviour()
    return _bare_ring(uavtrack.PrioritizedReplayRing, "ring1", 24, 5).with_behaviour()


def _register(name, buffer):
    for attr in ("_idx", "_w", "_rho_w", "priorities", "discounts", "log_mu"):
        t = getattr(buffer, attr, None)
        if t is not None:
            REC.known[f"{name}.{attr}"] = t
    for k, t in buffer.store.items():
        REC.known[f"{name}.store.{k}"] = t


def _digest(gen) -> str:
    return hashlib.sha1(gen.get_state().numpy().tobytes()).hexdigest()[:16]


def _seed(key: str) -> int:
    return int(hashlib.sha1(key.encode()).hexdigest()[:8], 16)


def run_case(key: str):
    which, path, option = key.split("|")
    REC.calls, REC.known, REC.fresh = [], {}, []
    learner = Learner()
    buffer = make_buffer(which)
    buffers = [buffer, make_partner(which)] if path == "update_from_many" else [buffer]
    for k, b in enumerate(buffers):
        _register(f"ring{k}", b)
    kw = dict(OPTIONS[option])
    if kw.get("rho_out"):
        outs = [torch.zeros(min(BATCH, b.count)) for b in buffers]
        for k, t in enumerate(outs):
            REC.known[f"rho_out{k}"] = t
        kw["rho_out"] = outs if path == "update_from_many" else outs[0]
    torch_buffer = isinstance(buffer, uavtrack.DeviceReplayBuffer)
    REC.dump = torch_buffer
    gen = None
    if torch_buffer:
        gen = kw["generator"] = torch.Generator().manual_seed(_seed(key))
    gathered = sharding.gather_learner_rows
    held = None
    try:
        if path == "update_from_many":
            held = learner.update_from_many(buffers, BATCH, **kw)
        elif path == "update_from_group":
            sharding.gather_learner_rows = lambda row, group=None: row.reshape(1, -1)
            held = learner.update_from(buffer, BATCH, group="group", **kw)
        else:
            held = getattr(learner, path)(buffer, BATCH, **kw)
    except Exception as e:                                            # errors are behaviour
        REC.calls.append(f"raised {type(e).__name__}: {e}")
    finally:
        sharding.gather_learner_rows = gathered
    lines = REC.calls
    del held
    if torch_buffer:
        lines.append("  generator " + _digest(gen))
        gen = torch.Generator().manual_seed(_seed(key))
        if isinstance(buffer, uavtrack.PrioritizedDeviceReplayBuffer):
            batch, idx, w = buffer.sample(BATCH, kw.get("beta", 0.4), generator=gen)
            lines.append(f"  sample() drew {json.dumps(idx.tolist())} {idx.dtype}")
            lines.append(f"  sample() weights {json.dumps(w.contiguous().view(torch.int32).tolist())} {w.dtype}")
        else:
            batch = buffer.sample(BATCH, generator=gen)
        lines.append(f"  sample() rows {json.dumps(batch['rewards'].to(torch.int64).tolist())}")
        lines.append("  sample() generator " + _digest(gen))
    return lines


def trace():
    return {key: run_case(key) for key in case_keys()}


def dump(cases) -> str:
    body = ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(line) for line in v) + "]" for k, v in cases.items())
    return "{\n" + body + "\n}\n"


def time_host(rounds: int = 5, calls: int = 2000):
    """Seconds per call of update_from and of update_from_many over eight rings (prioritised behaviour rings, importance
    and rho_bar on) against the recorder: the Python between the caller and the library."""
    learner = Learner()
    rings = [_bare_ring(uavtrack.PrioritizedReplayRing, f"ring{k}", 32, 20).with_behaviour() for k in range(8)]
    REC.known, REC.dump = {}, False
    out = {"update_from": [], "update_from_many": []}
    for _ in range(rounds):
        for what, fn, reps in (("update_from", lambda: learner.update_from(rings[0], BATCH, importance=True, rho_bar=1.0), calls),
                               ("update_from_many", lambda: learner.update_from_many(rings, BATCH, importance=True,
                                                                                     rho_bar=1.0), calls // 8)):
            fn()
            windows = []
            for _ in range(10):                                       # a round is its quietest window
                del REC.calls[:], REC.fresh[:]
                t0 = time.perf_counter()
                for _ in range(reps // 10):
                    fn()
                windows.append((time.perf_counter() - t0) / (reps // 10))
            out[what].append(min(windows))
    return out


if __name__ == "__main__":
    if "--record" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write(dump(trace()))
        print(f"recorded {len(case_keys())} cases into {GOLDEN}")
    elif "--time" in sys.argv:
        print(json.dumps({k: [round(1e6 * x, 2) for x in v] for k, v in time_host().items()}))
    else:
        sys.stdout.write(dump(trace()))
