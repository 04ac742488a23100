"""Reading tests/golden/f6_pmi_train.npz (tools/gen_pmi_trainer_golden.py).

fc1.weight is recorded at a seeded sample of its flat indices (<case>_w1_idx), every other tensor in full.  A "view"
is the 18 trainable tensors in PMINetwork.parameters() order, flattened, with fc1.weight reduced to that sample; the
recorded gradient magnitudes and Adam moments are views.  The initial state is rebuilt from the case's seed with
make_pmi_net (the same draws as the reference's constructor) and checked against its record."""
import json
import os

import numpy as np
import torch

from conftest import load_golden, GOLDEN
import pmi_trainer_mirror as mirror

W1 = mirror.param_names().index("fc1.weight")


def load():
    """-> (z, meta, rows): the fixture, its meta, and the observation history it was recorded on [1000, 12]."""
    z, meta = load_golden("f6_pmi_train")
    rows = np.load(os.path.join(GOLDEN, "f3_pmi_train.npz"))["train_data"]
    assert json.loads(str(np.load(os.path.join(GOLDEN, "f3_pmi_train.npz"))["meta"]))["n_uav"] == meta["n_uav"]
    return z, meta, rows


def indices(z, meta, case, call):
    """The call's index triples as int64: (t [b2], u [b2, 2])."""
    return z[f"{case}_c{call}_t"].astype(np.int64), z[f"{case}_c{call}_u"].astype(np.int64)


def initial_state(z, meta, case):
    """The full initial state_dict (numpy) of the case, rebuilt from its seed; raises if it is not the recorded one."""
    import uavtrack
    torch.manual_seed(meta["cases"][case]["seed"])
    sd = {k: v.numpy().copy() for k, v in uavtrack.make_pmi_net(meta["cases"][case]["hidden"]).state_dict().items()}
    assert list(sd) == mirror.state_names()
    idx = z[f"{case}_w1_idx"]
    for k, v in sd.items():
        rec = z[f"{case}_sd0_{k}"]
        got = v.reshape(-1)[idx] if k == "fc1.weight" else v
        assert np.array_equal(np.asarray(got), rec), f"{case}: the rebuilt initial {k} is not the recorded one"
    return sd


def view(sd, z, case):
    """The view of a full state dict's trainable tensors (float64)."""
    idx = z[f"{case}_w1_idx"]
    return np.concatenate([np.asarray(sd[k], np.float64).reshape(-1)[idx] if k == "fc1.weight"
                           else np.asarray(sd[k], np.float64).ravel() for k in mirror.param_names()])


def view_flat(flat, H, z, case):
    """The view of a full flat array in parameters() order (gradients, Adam moments)."""
    sizes = [np.asarray(v).size for v in _shapes(H)]
    parts = np.split(np.asarray(flat), np.cumsum(sizes)[:-1])
    parts[W1] = parts[W1][z[f"{case}_w1_idx"]]
    return np.concatenate(parts)


def recorded(z, case, call):
    """The view of the state recorded after a call (float64)."""
    return np.concatenate([z[f"{case}_c{call}_sd_{k}"].astype(np.float64).ravel() for k in mirror.param_names()])


def _shapes(H):
    shapes = []
    for k in (5, 4, 3, 3 * H):
        shapes += [np.empty((H, k)), np.empty(H), np.empty(H), np.empty(H)]
    return shapes + [np.empty((1, H)), np.empty(1)]
