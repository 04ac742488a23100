"""The layout of csrc/: which translation unit reaches which project header, and every header compiling on its own.

A change to the learner, the trainer, the replay ring or the episode results must not recompile the rollout kernel or
the MAAC-R scorer (minutes each), and those four subsystems see nothing of the environment.  The first two tests read
the `#include "..."` lines alone (no compiler, no generated code); the third compiles each header by itself."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "marl-uavs-targets-tracking_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)

ENV_SIDE = ("step_kernel", "pmi_kernel", "policy_kernel", "reset_kernel", "actor_pack_kernel", "pmi_pack_kernel")
ENV_SIDE_MAY_NOT_REACH = ("adam.h", "learner.h", "pmi_train.h", "replay.h", "episode.h")      # ... and any api_*.h
ENV_FREE = ("learner_kernel", "pmi_train_kernel", "replay_kernel", "episode_kernel", "api_replay", "api_episode")
ENV_FREE_MAY_NOT_REACH = ("env.h", "actor.h", "greedy.h", "pmi_pack.h")


def direct_includes():
    """{file name: the project files it names in #include "..."} over csrc/*.hip and csrc/*.h; a quoted include that is
    neither in csrc/ nor in include/ fails here."""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            named = _INCLUDE.findall(f.read())
        for inc in named:
            assert os.path.exists(os.path.join(CSRC, inc)) or os.path.exists(os.path.join(INCLUDE, inc)), \
                f'{name} includes "{inc}", which is neither in csrc/ nor in include/'
        out[name] = [inc for inc in named if os.path.exists(os.path.join(CSRC, inc))]
    return out


def closure(name, direct):
    assert name in direct, f"csrc/{name} does not exist"
    seen, todo = set(), list(direct[name])
    while todo:
        inc = todo.pop()
        if inc not in seen:
            seen.add(inc)
            todo.extend(direct[inc])
    return seen


def headers():
    return sorted(n for n in os.listdir(CSRC) if n.endswith(".h"))


def test_env_side_kernels_reach_no_trainer_replay_episode_or_abi_header():
    direct = direct_includes()
    for unit in ENV_SIDE:
        reached = closure(unit + ".hip", direct)
        bad = sorted(h for h in reached if h in ENV_SIDE_MAY_NOT_REACH or re.fullmatch(r"api_.*\.h", h))
        assert not bad, f"{unit}.hip reaches {bad} (through {sorted(reached)})"


def test_trainer_replay_and_episode_units_reach_nothing_of_the_environment():
    direct = direct_includes()
    for unit in ENV_FREE:
        reached = closure(unit + ".hip", direct)
        bad = sorted(h for h in reached if h in ENV_FREE_MAY_NOT_REACH)
        assert not bad, f"{unit}.hip reaches {bad} (through {sorted(reached)})"


@pytest.mark.parametrize("header", headers())
def test_header_compiles_on_its_own(header):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-x", "hip", "-Wno-pragma-once-outside-header",
           "-I" + INCLUDE, "-I" + CSRC, os.path.join(CSRC, header)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"{header} does not compile on its own:\n{r.stdout}"
