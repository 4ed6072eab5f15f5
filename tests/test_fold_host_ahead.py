"""The sequential merge fold with its host planning taken off the device's chain (hmsg_merge.hip + hmsg_fold_host.h: the box
table and the cloud list kept in place from step to step, the next frame's pairs enumerated while a step's DBSCAN batch runs and
merged with the pairs of the batch's outputs afterwards) against the fold as it was (HMSG_FOLD_HOST_AHEAD=0: every pair
enumerated at the start of the step, the list rebuilt per step).  The pair list is the same list in the same order, so the
overlap pack, the components and the instances are the same -- with the fold beside the fusion or inside hmsg_merge_instances,
with collections of the point pool forced, and with HMSG_DEBUG_FOLD_PAIRS_CHECK=1, which computes the reference list as well
every step and fails the call on any difference."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import parity_common as PC
from tests.test_fold_pipeline import _device_scene, _host_scene

_SWITCHES = ("HMSG_FOLD_HOST_AHEAD", "HMSG_DEBUG_FOLD_PAIRS_CHECK", "HMSG_DEBUG_GC_POINTS", "HMSG_DEBUG_TIMING")


def _env(ahead, check, gc, timing=False):
    env = {}
    if not ahead:
        env["HMSG_FOLD_HOST_AHEAD"] = "0"
    if check:
        env["HMSG_DEBUG_FOLD_PAIRS_CHECK"] = "1"
    if gc:
        env["HMSG_DEBUG_GC_POINTS"] = "1"      # (a collection as often as the fold allows one)
    if timing:
        env["HMSG_DEBUG_TIMING"] = "1"
    return env


def _pair_list_counts(err):
    m = re.findall(r"pair lists: (\d+) steps merged from an ahead and a late part, (\d+) enumerated whole", err)
    assert m, err
    return int(m[-1][0]), int(m[-1][1])


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
@pytest.mark.parametrize("nopipe,gc", [(True, False), (True, True), (False, False), (False, True)])
def test_fold_host_ahead_equals_the_former_fold_on_the_simulator(capfd, nopipe, gc):
    """(one case per (fold inside hmsg_merge_instances / beside the fusion, collections forced or not): the cases run on different
    workers of the CPU suite, each against its own run of the former fold)"""
    from holoagent_amd._lib import HmsgLib
    from holoagent_amd.synth import SceneSpec, SynthScene
    for k in _SWITCHES:
        assert k not in os.environ, k
    L = HmsgLib(PC.EMU_PATH)
    spec = SceneSpec(seed=5, rooms_x=1, rooms_z=1, room_size=(3.6, 2.5, 3.2), objects_per_room=4, width=64, height=48,
                     n_frames=8, n_masks=5, feat_dim=16)
    scn = SynthScene(spec)
    frames = [scn.frame(i) for i in range(spec.n_frames)]
    ref, ref_f = _host_scene(L, frames, 16, nopipe=True, env=_env(ahead=False, check=False, gc=False))
    assert len(ref) >= 3
    capfd.readouterr()
    counts = {}
    for check, ahead in itertools.product((False, True), (False, True)):
        if nopipe and not gc and not check and not ahead:
            continue                                        # (the reference run itself)
        got, got_f = _host_scene(L, frames, 16, nopipe=nopipe, split=not nopipe, env=_env(ahead, check, gc, timing=True))
        what = (nopipe, gc, check, ahead)
        assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref)), what
        assert np.array_equal(got_f, ref_f), what
        counts[(check, ahead)] = _pair_list_counts(capfd.readouterr().err)
    # The planned fold did plan.  Eight frames are seven fold steps and the final pass: the first step and the final pass have
    # nothing ahead of them, the six between do -- unless a collection of the pool came between (forced collections take ahead
    # parts away again) or, beside the fusion, the frame was not there yet.  The former fold never goes through the planner.
    for (check, ahead), (merged, whole) in counts.items():
        if not ahead:
            assert (merged, whole) == (0, 0)
            continue
        assert merged + whole == spec.n_frames, (nopipe, gc, check, ahead, merged, whole)
        if gc:
            assert 0 < merged < spec.n_frames - 2, (nopipe, gc, check, ahead, merged, whole)
        elif nopipe:
            assert (merged, whole) == (spec.n_frames - 2, 2)
        else:
            assert merged > 0


@pytest.mark.gpu
def test_fold_host_ahead_equals_the_former_fold_on_the_gpu():
    """configs[1]'s scene (device-rendered, 640x480, 32 masks per frame), 130 frames: two fusion batches and a bit, so the fold
    beside the fusion meets "the next frame is not there yet" at the batch ends, and the walk crosses the first room change at
    frame 125.  SHA-1 of the instances and the pooled features: the former fold, the planned fold inside hmsg_merge_instances
    and beside the fusion, and the planned fold with the reference list checked every step."""
    import torch
    import bench
    from holoagent_amd._lib import HmsgLib
    from holoagent_amd.synth import SceneSpec
    for k in _SWITCHES:
        assert k not in os.environ, k
    L = HmsgLib()
    spec = SceneSpec(seed=1234, n_frames=130, feat_dim=64, n_masks=32)
    inp = bench.build_scene_inputs(L, spec, torch.device("cuda", 0), torch)
    ref = _device_scene(L, spec, inp, nopipe=True, env=_env(ahead=False, check=False, gc=False))
    assert ref[0][0] > 10
    assert _device_scene(L, spec, inp, nopipe=False) == ref
    assert _device_scene(L, spec, inp, nopipe=True) == ref
    assert _device_scene(L, spec, inp, nopipe=True, env=_env(ahead=True, check=True, gc=False)) == ref
    assert _device_scene(L, spec, inp, nopipe=False, env=_env(ahead=True, check=True, gc=False)) == ref
