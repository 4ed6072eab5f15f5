"""The query applications' flow from C (tests/host_c/hmsg_host_rooms.c, strict C99 against include/hmsg.h ALONE): hmsg_load ->
hmsg_graph_name_rooms (obj_embedding) -> room_name_emb formed from type_of_room -> label-mode hmsg_graph_query -> hmsg_graph_to_json,
compared with the same steps through the Python binding.  The graph directory is the synthetic scene of
tests/test_scene_graph_cabi.py, built and saved through the library.  CPU: the kernel simulator; -m gpu: libhmsg.so."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import parity_common as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_c", "hmsg_host_rooms.c")
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "holoagent_amd", "libhmsg.so")
TYPES = ["Pantry", "Office", "Office-Pantry"]


def _compile(lib_path, out):
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", INC, SRC, "-o", out, lib_path,
           "-Wl,-rpath," + os.path.dirname(lib_path), "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def _run(lib_path, device, tmp_path):
    from holoagent_amd._lib import HmsgLib, SceneGraph
    from tests.test_scene_graph_cabi import _build, _rest
    L = HmsgLib(lib_path)
    spec, inp, sc = _build(L, device)
    F, D = spec.n_frames, spec.feat_dim
    poses = np.stack([np.asarray(inp["pose"][i], np.float64).reshape(4, 4) for i in range(F)])
    cg = SceneGraph.begin(sc, poses, inp["f_g"].cpu().numpy(), poses_inv=np.linalg.inv(poses), num_views=5, host_threads=2)
    _rest(sc, inp)
    cg.finish(None, None)
    gdir = tmp_path / "graph"
    cg.save(gdir)
    cg.close()
    sc.close()
    rng = np.random.Generator(np.random.PCG64(31))
    T = rng.standard_normal((len(TYPES), D)).astype(np.float32)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    Q, C, k = 5, 2, 3
    T_obj = rng.standard_normal((Q, C, D)).astype(np.float32)
    T_obj /= np.linalg.norm(T_obj, axis=-1, keepdims=True)
    T_room = np.ascontiguousarray(T[np.arange(Q) % len(TYPES)])
    fin = tmp_path / "in.bin"
    with open(fin, "wb") as f:
        np.array([len(TYPES), D, Q, C, k], np.int32).tofile(f)
        for a in (T, T_obj, T_room):
            np.ascontiguousarray(a, np.float32).tofile(f)
    exe = _compile(lib_path, str(tmp_path / "hmsg_host_rooms"))
    fout, fjson = tmp_path / "out.bin", tmp_path / "out.json"
    r = subprocess.run([exe, str(gdir), str(fin), str(fout), str(fjson)] + TYPES, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr
    raw = open(fout, "rb").read()
    R = int(np.frombuffer(raw[:4], np.int32)[0])
    RM = max(R, 10)
    a = np.frombuffer(raw[4:], np.uint8)
    cur = [0]

    def take(dt, n):
        b = a[cur[0]: cur[0] + n * np.dtype(dt).itemsize].view(dt)
        cur[0] += n * np.dtype(dt).itemsize
        return b
    t_c = take(np.int32, R)
    nsel_c = take(np.int32, Q)
    sel_c = take(np.int32, Q * RM).reshape(Q, RM)
    idx_c, room_c, score_c = take(np.int32, Q * k).reshape(Q, k), take(np.int32, Q * k).reshape(Q, k), take(np.float64, Q * k).reshape(Q, k)
    # ---- the same steps through the binding
    lg = SceneGraph.load(gdir, lib_=L)
    t_py = lg.name_rooms("obj_embedding", T, TYPES)
    sel, idx, room, score = lg.query(T_obj, np.zeros(Q, np.int32), T_room, np.full(Q, -1, np.int32), np.ones(Q, np.int32), k,
                                     room_name_emb=np.ascontiguousarray(T[t_py].astype(np.float64)))
    assert R >= 1 and np.array_equal(t_c, t_py)
    assert [sel_c[q, : nsel_c[q]].tolist() for q in range(Q)] == sel
    assert np.array_equal(idx_c, idx) and np.array_equal(room_c, room) and np.array_equal(score_c, score)
    assert [r_["name"] for r_ in json.load(open(fjson))["rooms"]] == [TYPES[t] for t in t_py] == [r_["name"] for r_ in lg.rooms()]
    lg.close()


@pytest.mark.skipif(not os.path.exists(PC.EMU_PATH), reason="kernel simulator not built")
def test_c_host_rooms_on_the_simulator(tmp_path):
    import torch
    _run(PC.EMU_PATH, torch.device("cpu"), tmp_path)


@pytest.mark.gpu
def test_c_host_rooms_gpu(tmp_path):
    import torch
    _run(LIB, torch.device("cuda", 0), tmp_path)
