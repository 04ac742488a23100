"""The reference's PMINetwork training surface (src/models/PMINet.py:20-109) on the device: one `train_pmi` is ONE
library call (uavtrack_pmi_trainer_train) -- every mini-batch step's gather, both train-mode forwards, CustomLoss,
the backward pass and the torch.optim.Adam step -- stream-ordered, with no synchronisation and no allocation inside
the library.  The (timestep, uav-pair) triples are drawn as `sample_pmi_pairs` draws them, so under the same
torch.manual_seed the trainer selects the reference's rows; the rows themselves are gathered in the kernels.

state_dict / save / load speak the reference's formats (30 state_dict keys; {'model_state_dict',
'optimizer_state_dict'} checkpoints under <save_dir>/pmi/), and `BatchedUavEnv.set_pmi(trainer)` folds and uploads
the trained network to the MAAC-R scorer."""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import adam
from ._handle import Handle, current_device
from ._lib import host_ptr, ptr as _ptr
from .adam import flat, from_state_dict, to_state_dict
from .pmi import fold_pmi_state_dict, make_pmi_net

_BN = ("bn_comm", "bn_obs", "bn_boundary_state", "bn1")


class DevicePMINetwork(Handle):
    """PMINetwork(hidden_dim=hidden_dim, b2_size=b2_size) with train_pmi on the GPU.  Initial weights are
    torch.nn.Linear's defaults drawn from torch's global generator in the reference's layer order, so under the same
    seed they are the reference's; the learning rate defaults to the reference's Adam(lr=0.001) (PMINet.py:39)."""
    _prefix = "uavtrack_pmi_trainer_"

    def __init__(self, hidden_dim: int = 64, b2_size: int = 3000, device="cuda:0", lr: float = 1e-3,
                 max_batch: int = 0):
        self.device = current_device(device)
        self.hidden_dim, self.b2_size, self.lr = int(hidden_dim), int(b2_size), float(lr)
        if not 1 <= self.hidden_dim <= 256:
            raise ValueError(f"hidden_dim must be in [1, 256], got {hidden_dim}")
        self._net = make_pmi_net(self.hidden_dim)      # host-side module: layout, initialisation, state_dict format
        self._create(_lib.PmiTrainerConfig(device_id=self.device.index, hidden=self.hidden_dim, pad_=0,
                                           max_batch=int(max_batch), lr=self.lr))
        ns, nt = C.c_int64(), C.c_int64()
        _lib.check(self._lib.uavtrack_pmi_trainer_num_params(self._h, C.byref(ns), C.byref(nt)),
                   "uavtrack_pmi_trainer_num_params")
        self.num_state, self.num_params = ns.value, nt.value
        self.load_state_dict(self._net.state_dict())

    def reserve(self, max_batch: int) -> None:
        """Scratch for mini-batches of up to max_batch rows (a larger batch_size is an error; the default is 4096)."""
        _lib.check(self._lib.uavtrack_pmi_trainer_reserve(self._h, int(max_batch)), "uavtrack_pmi_trainer_reserve")

    def check(self) -> None:
        """Synchronises; raises if a train call since the last check was refused on the device (an index out of
        range), which then changed nothing."""
        self._check()

    # ---- training
    def train_indices(self, rows: torch.Tensor, n_uav: int, t_idx: torch.Tensor, u_idx: torch.Tensor,
                      batch_size: int, avg_loss: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None,
                      outputs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """train_pmi after its index draw: rows [T * n_uav, 12] fp32, t_idx [b2] and u_idx [b2, 2] int64, all
        contiguous on this trainer's device.  Optional outputs (device, fp32): losses [b2 // batch_size] (|loss| per
        step), outputs [b2 // batch_size, 2, batch_size] (output_1_2, output_1_3).  Returns avg_loss, a device
        scalar, without synchronising.  Fixed shapes and no allocation when avg_loss is given: capturable."""
        b2 = int(t_idx.numel())
        for name, t, dt in (("rows", rows, torch.float32), ("t_idx", t_idx, torch.int64), ("u_idx", u_idx, torch.int64)):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} tensor on {self.device}")
        if rows.dim() != 2 or rows.shape[1] != _lib.OBS_DIM:
            raise ValueError(f"rows must be [T * n_uav, {_lib.OBS_DIM}], got {tuple(rows.shape)}")
        if tuple(u_idx.shape) != (b2, 2):
            raise ValueError(f"u_idx must be [{b2}, 2], got {tuple(u_idx.shape)}")
        nb = b2 // int(batch_size) if batch_size > 0 else 0
        for name, t, shape in (("losses", losses, (nb,)), ("outputs", outputs, (nb, 2, int(batch_size)))):
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()
                                  or tuple(t.shape) != shape):
                raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor on {self.device}")
        if avg_loss is None:
            avg_loss = torch.empty((), device=self.device)
        _lib.check(self._lib.uavtrack_pmi_trainer_train(
            self._h, _ptr(rows), int(rows.shape[0]), int(n_uav), _ptr(t_idx), _ptr(u_idx), b2, int(batch_size),
            _ptr(avg_loss), _ptr(losses), _ptr(outputs), self._stream()), "uavtrack_pmi_trainer_train")
        return avg_loss

    def _draw(self, groups: int, n_uav: int, generator: Optional[torch.Generator]):
        """train_pmi's index draw over `groups` timesteps, in the reference's order (PMINet.py:76-77)."""
        draw_dev = generator.device if generator is not None else torch.device("cpu")
        t_idx = torch.randint(low=0, high=groups, size=(self.b2_size,), device=draw_dev, generator=generator)
        u_idx = torch.randint(low=0, high=int(n_uav), size=(self.b2_size, 2), device=draw_dev, generator=generator)
        return t_idx, u_idx

    def train_pmi(self, config, train_data: torch.Tensor, n_uav: int, generator: Optional[torch.Generator] = None,
                  sync: bool = True, group=None, group_counts=None):
        """PMINetwork.train_pmi (PMINet.py:74-100): train_data [T * n_uav, 12] or [T, (B,) n_uav, 12] observations on
        the device; config["pmi"]["batch_size"].  The index triples come from torch's CPU generator (the global one
        unless `generator` is given; a device generator keeps the draw on the device) in the reference's order.
        Returns avg_loss as a float (sync=True) or a device scalar.

        group (a torch.distributed process group): data parallelism over its ranks.  The timeline is the ranks'
        histories in rank order; group rank 0 draws the triples over all of it and broadcasts them (the other ranks'
        generators are not used), every rank selects the rows of the draws that fall into its own history
        (uavtrack_pmi_trainer_select), ONE all-gather (gather_pmi_selected) hands every rank all the selected rows, and
        every rank then runs the same whole train_indices on them: the mini-batch and its BatchNorm statistics are not
        split.  Ranks that start equal (broadcast_pmi_trainer) end with the same bits, those of one process calling
        train_indices on the concatenated history with the same triples.  Triples out of range (rank 0's randint draws
        none) refuse the call on every rank's device, as on one process: nothing changes, the loss is NaN, check()
        reports it.  group_counts: the ranks' timestep counts, if
        the caller knows them (otherwise one small all-gather per call exchanges them)."""
        bs = int(config["pmi"]["batch_size"])
        rows = train_data.reshape(-1, _lib.OBS_DIM)
        if rows.device != self.device:
            raise ValueError(f"train_data must be on {self.device}")
        rows = rows.to(torch.float32).contiguous()
        if rows.shape[0] % int(n_uav) != 0:
            raise ValueError(f"train_data has {rows.shape[0]} rows, not a multiple of n_uav = {n_uav}")
        T = rows.shape[0] // int(n_uav)
        if group is not None:
            avg = self._train_pmi_group(rows, T, int(n_uav), bs, generator, group, group_counts)
            return float(avg) if sync else avg
        t_idx, u_idx = self._draw(T, n_uav, generator)
        avg = self.train_indices(rows, int(n_uav), t_idx.to(self.device).contiguous(), u_idx.to(self.device).contiguous(),
                                 bs)
        return float(avg) if sync else avg

    # ---- several histories: K shards on this device, or one rank's part of a process group's timeline
    def _sources(self, sources, n_uav: int):
        """(the ctypes source table, the [-1, 12] views it points into, total timesteps) of a list of histories."""
        sources = list(sources)
        if not 1 <= len(sources) <= _lib.PMI_MAX_SOURCES:
            raise ValueError(f"sources must hold 1 to {_lib.PMI_MAX_SOURCES} tensors, got {len(sources)}")
        views, table = [], (_lib.PmiSource * len(sources))()
        for k, s in enumerate(sources):
            if s.device != self.device or s.dtype != torch.float32 or not s.is_contiguous():
                raise ValueError(f"sources[{k}] must be a contiguous torch.float32 tensor on {self.device}")
            if s.numel() == 0 or s.numel() % (_lib.OBS_DIM * int(n_uav)) != 0:
                raise ValueError(f"sources[{k}] has {s.numel()} floats, not a positive multiple of n_uav = {n_uav} rows "
                                 f"of {_lib.OBS_DIM}")
            v = s.reshape(-1, _lib.OBS_DIM)
            views.append(v)
            table[k].rows, table[k].n_rows = v.data_ptr(), v.shape[0]
        return table, views, sum(v.shape[0] for v in views) // int(n_uav)

    def train_indices_many(self, sources, n_uav: int, t_idx: torch.Tensor, u_idx: torch.Tensor, batch_size: int,
                           avg_loss: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None,
                           outputs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """train_indices on the timeline of `sources`, a list of 1 to 64 contiguous fp32 device tensors, each taken as
        [-1, 12] rows (a positive multiple of n_uav): timestep t of the timeline is timestep t - base_k of the source
        k whose span holds it, base_k the timesteps of the sources before it.  Bit for bit
        train_indices(torch.cat(sources), ...), without the concatenation: the selected rows are gathered by one
        kernel of the same library call (uavtrack_pmi_trainer_train_many).  Capturable like train_indices; the source
        tensors' addresses and sizes are captured by value."""
        b2 = int(t_idx.numel())
        for name, t in (("t_idx", t_idx), ("u_idx", u_idx)):
            if t.device != self.device or t.dtype != torch.int64 or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous torch.int64 tensor on {self.device}")
        if tuple(u_idx.shape) != (b2, 2):
            raise ValueError(f"u_idx must be [{b2}, 2], got {tuple(u_idx.shape)}")
        table, views, _ = self._sources(sources, n_uav)
        nb = b2 // int(batch_size) if batch_size > 0 else 0
        for name, t, shape in (("losses", losses, (nb,)), ("outputs", outputs, (nb, 2, int(batch_size)))):
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()
                                  or tuple(t.shape) != shape):
                raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor on {self.device}")
        if avg_loss is None:
            avg_loss = torch.empty((), device=self.device)
        _lib.check(self._lib.uavtrack_pmi_trainer_train_many(
            self._h, table, len(views), int(n_uav), _ptr(t_idx), _ptr(u_idx), b2, int(batch_size), _ptr(avg_loss),
            _ptr(losses), _ptr(outputs), self._stream()), "uavtrack_pmi_trainer_train_many")
        return avg_loss

    def train_pmi_many(self, config, sources, n_uav: int, generator: Optional[torch.Generator] = None,
                       sync: bool = True):
        """train_pmi over several histories (the K `res["obs"]` of K shard handles) without concatenating them: the
        triples are drawn over the total timestep count exactly as train_pmi draws them, then train_indices_many.
        Under the same generator state it is bit for bit
        train_pmi(config, torch.cat([s.reshape(-1, 12) for s in sources]), n_uav).

        The timeline of K shards is shard-major: all of shard 0's timesteps, then shard 1's.  It is therefore NOT the
        row order of the unsharded batch's [T, B, N, 12], and the same seed selects other rows than an unsharded run
        would (every row is still drawn with the same probability)."""
        _, _, groups = self._sources(sources, n_uav)
        t_idx, u_idx = self._draw(groups, n_uav, generator)
        avg = self.train_indices_many(sources, int(n_uav), t_idx.to(self.device).contiguous(),
                                      u_idx.to(self.device).contiguous(), int(config["pmi"]["batch_size"]))
        return float(avg) if sync else avg

    def _select(self, sources, group_base: int, total_groups: int, n_uav: int, t_idx: torch.Tensor, u_idx: torch.Tensor,
               selected: torch.Tensor) -> torch.Tensor:
        """The gather alone (uavtrack_pmi_trainer_select): `sources` are timesteps [group_base, group_base + their
        count) of a timeline of total_groups; for every draw i inside that span selected[i] ([b2, 2, 12] fp32, device,
        contiguous) receives rows (t_idx[i], u_idx[i][0]) and (t_idx[i], u_idx[i][1]); other draws' rows stay as they
        are.  A draw outside the timeline makes the call write nothing, and check() reports it."""
        b2 = int(t_idx.numel())
        for name, t, dt, shape in (("t_idx", t_idx, torch.int64, (b2,)), ("u_idx", u_idx, torch.int64, (b2, 2)),
                                   ("selected", selected, torch.float32, (b2, 2, _lib.OBS_DIM))):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
        table, views, _ = self._sources(sources, n_uav)
        _lib.check(self._lib.uavtrack_pmi_trainer_select(
            self._h, table, len(views), int(group_base), int(total_groups), int(n_uav), _ptr(t_idx), _ptr(u_idx), b2,
            _ptr(selected), self._stream()), "uavtrack_pmi_trainer_select")
        return selected

    def _train_pmi_group(self, rows, T: int, n_uav: int, bs: int, generator, group, group_counts):
        import torch.distributed as dist
        from .sharding import _pmi_owner_triples, gather_pmi_selected
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        staged = dist.get_backend(group) == "gloo"                    # gloo: collectives on host tensors
        wire = torch.device("cpu") if staged else self.device
        if group_counts is None:
            counts = torch.empty(world, dtype=torch.int64, device=wire)
            dist.all_gather_into_tensor(counts, torch.tensor([T], dtype=torch.int64, device=wire), group=group)
            group_counts = counts.tolist()
        group_counts = [int(c) for c in group_counts]
        if len(group_counts) != world or group_counts[rank] != T or min(group_counts) < 1:
            raise ValueError(f"group_counts {group_counts}: one positive timestep count per rank, this rank's being {T}")
        total, b2 = sum(group_counts), self.b2_size
        if rank == 0:
            t_idx, u_idx = self._draw(total, n_uav, generator)
            triples = torch.cat([t_idx.reshape(-1, 1), u_idx], dim=1).to(wire).contiguous()
        else:
            triples = torch.empty((b2, 3), dtype=torch.int64, device=wire)
        dist.broadcast(triples, src=dist.get_global_rank(group, 0), group=group)
        triples = triples.to(self.device)
        t_idx, u_idx = triples[:, 0].contiguous(), triples[:, 1:].contiguous()
        mine = torch.zeros((b2, 2, _lib.OBS_DIM), device=self.device)
        self._select([rows], sum(group_counts[:rank]), total, n_uav, t_idx, u_idx, mine)
        block = gather_pmi_selected(mine, group)                      # [world * b2, 2, 12], rank-major
        t2, u2 = _pmi_owner_triples(t_idx, u_idx, group_counts, n_uav)    # all -1 if any draw is out of range
        return self.train_indices(block.reshape(-1, _lib.OBS_DIM), 2, t2, u2, bs)

    def publish_pmi(self, env) -> None:
        """This trainer's current network into env's MAAC-R scorer, folded and packed on the device
        (uavtrack_pmi_trainer_publish): stream-ordered, no host copy, no synchronisation, capturable; bit for bit what
        `env.set_pmi(self)` installs.  env must hold weights of this hidden width (set_pmi once, before the loop)."""
        _lib.check(self._lib.uavtrack_pmi_trainer_publish(self._h, env._h, self._stream()),
                   "uavtrack_pmi_trainer_publish")

    # ---- state
    def _get(self):
        st = np.empty(self.num_state, np.float32)
        nbt = np.empty(_lib.PMI_BN_LAYERS, np.int64)
        _lib.check(self._lib.uavtrack_pmi_trainer_get_params(self._h, host_ptr(st), host_ptr(nbt), st.size, self._stream()),
                   "uavtrack_pmi_trainer_get_params")
        return st, nbt

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The reference PMINetwork's state_dict (30 keys, its order; CPU tensors)."""
        st, nbt = self._get()
        sd, o = OrderedDict(), 0
        for k, v in self._net.state_dict().items():
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.tensor(int(nbt[_BN.index(k.split(".")[0])]), dtype=torch.int64)
            else:
                sd[k] = torch.from_numpy(st[o:o + v.numel()].copy()).view_as(v)
                o += v.numel()
        return sd

    def load_state_dict(self, sd) -> None:
        """PMINetwork.load_state_dict: torch checks keys and shapes first; the Adam state stays as it is."""
        probe = make_pmi_net(self.hidden_dim)
        probe.load_state_dict(sd)
        items = probe.state_dict()
        st = flat(v for k, v in items.items() if not k.endswith("num_batches_tracked"))
        nbt = np.array([int(items[b + ".num_batches_tracked"]) for b in _BN], np.int64)
        _lib.check(self._lib.uavtrack_pmi_trainer_set_params(self._h, host_ptr(st), host_ptr(nbt), st.size, self._stream()),
                   "uavtrack_pmi_trainer_set_params")

    def optimizer_state(self):
        """(exp_avg [P], exp_avg_sq [P], step [18]) as numpy arrays, parameters() order."""
        return adam.read(self._lib.uavtrack_pmi_trainer_get_optimizer_state, self._h, self.num_params,
                         _lib.PMI_TRAIN_TENSORS, self._stream())

    def optimizer_state_dict(self) -> dict:
        """torch.optim.Adam(PMINetwork.parameters(), lr).state_dict() of this trainer, built by torch itself."""
        return to_state_dict(self._net.parameters(), self.lr, *self.optimizer_state())

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """optimizer.load_state_dict: a torch.optim.Adam state_dict over PMINetwork.parameters().  (The learning rate
        stays the one this trainer was built with.)"""
        mf, vf, steps = from_state_dict(make_pmi_net(self.hidden_dim).parameters(), self.lr, sd)
        adam.write(self._lib.uavtrack_pmi_trainer_set_optimizer_state, self._h, mf, vf, steps, self._stream())

    def save(self, save_dir: str, epoch_i) -> None:
        """PMINetwork.save (PMINet.py:102-106): <save_dir>/pmi/pmi_weights_<epoch>.pth holding
        {'model_state_dict', 'optimizer_state_dict'}."""
        os.makedirs(os.path.join(save_dir, "pmi"), exist_ok=True)
        torch.save({"model_state_dict": self.state_dict(), "optimizer_state_dict": self.optimizer_state_dict()},
                   os.path.join(save_dir, "pmi", f"pmi_weights_{epoch_i}.pth"))

    def load(self, path: Optional[str]) -> None:
        """PMINetwork.load (PMINet.py:108-112): a checkpoint that exists replaces the weights and the Adam state."""
        if path and os.path.exists(path):
            ck = torch.load(path, map_location="cpu")
            self.load_state_dict(ck["model_state_dict"])
            self.load_optimizer_state_dict(ck["optimizer_state_dict"])

    def folded(self):
        """(blob, hidden): the BatchNorm-folded eval-mode network uavtrack_set_pmi_weights takes."""
        return fold_pmi_state_dict(self.state_dict())
