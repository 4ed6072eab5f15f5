"""Golden generator for the room naming: runs the REFERENCE's own Graph.generate_room_names (graph.py:2146-2187) with
generate_method="obj_embedding" (Room.infer_room_type_from_objects, room.py:237-308 -> feats_denoise_dbscan, utils/graph_utils.py:682-728,
scikit-learn's DBSCAN) and "view_embedding" (room.py:131-172) on a synthetic graph, then its label-mode room query and object query,
and stores inputs + answers as tests/golden/roomnames_obj.npz.  Nothing of the reference travels: only data.

    python scripts/gen_golden_room_names.py            # from the repo root, where the reference checkout exists

The reference is imported with the recipe of oracle/refdrive/gen_golden.py; get_text_feats_multiple_templates is
replaced in BOTH graph.py and room.py (room.py imports it by name) by a deterministic table, and the Graph is made with __new__ as
gen_golden.py does for query.npz.  The rooms are drawn until every pairwise cosine distance inside a room lies at least 1e-4 away from
eps = 0.02 and every room's best type score at least 1e-6 above the runner-up, in float32 and in float64 (room names).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

EPS, DIST_MARGIN, SCORE_MARGIN = 0.02, 1e-4, 1e-6
TYPES = ["Pantry", "Office", "Office-Pantry"]          # the sh3f application's default_room_types
D = 32


def make_rooms(rng, T):
    """[(objects [n, D] f64, views [v, D] f64)], one per case of the issue's list"""
    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    def cluster(centre, n, s=0.012):
        return unit(centre)[None] + s * rng.standard_normal((n, D))

    def far(n):
        return rng.standard_normal((n, D))

    def near_type(t, s=0.6):
        return T[t] + s * rng.standard_normal(D) / np.sqrt(D)

    rooms = []
    rooms.append(far(5))                                                         # 0 all noise
    x = np.concatenate([cluster(near_type(1), 6), far(3)])                       # 1 one cluster + outliers
    rooms.append(x[rng.permutation(len(x))])
    a, b = cluster(near_type(0), 4), cluster(near_type(2), 4)                    # 2 two equal clusters (the tie)
    rooms.append(np.concatenate([far(1), b[:1], a[:2], b[1:], a[2:]]))
    rooms.append(far(1))                                                         # 3 a single object
    rooms.append(np.concatenate([np.zeros((2, D)), far(1)]))                     # 4 two zero rows + one other
    parts = [cluster(near_type(int(rng.integers(0, 3))), int(n)) for n in rng.integers(18, 32, 12)]   # 5 ~300 objects, 12 clusters
    x = np.concatenate(parts + [far(10)])
    rooms.append(x[rng.permutation(len(x))])
    x = np.concatenate([cluster(near_type(0), 7), far(2)])                       # 6 objects say type 0, the views type 2
    rooms.append(x)
    views = [np.stack([near_type(int(rng.integers(0, 3)), 0.9) for _ in range(int(rng.integers(2, 6)))]) for _ in rooms]
    views[6] = np.stack([near_type(2, 0.3) for _ in range(4)])
    return [(o, v) for o, v in zip(rooms, views)]


def margins_ok(rooms, T):
    for objs, views in rooms:
        for dt in (np.float32, np.float64):
            x = objs.astype(dt).astype(np.float64)
            nrm = np.linalg.norm(x, axis=1, keepdims=True)
            nrm[nrm == 0] = 1
            xn = x / nrm
            d = 1 - xn @ xn.T
            np.fill_diagonal(d, 0)
            if np.any(np.abs(d - EPS) < DIST_MARGIN):
                return False
        for v in views:
            s = np.sort(v @ T.T.astype(np.float64))
            if s[-1] - s[-2] < SCORE_MARGIN:
                return False
    return True


def main():
    from oracle.refdrive.gen_golden import import_reference
    G, _ = import_reference()
    import memory.hmsg.graph.room as R
    rng = np.random.Generator(np.random.PCG64(2026))
    words = TYPES + ["background"] + ["thing%d" % i for i in range(6)]
    table = {}
    for w in words:
        t = rng.standard_normal((2, D)).astype(np.float32)
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        table[w] = t.mean(axis=0)
    T = np.stack([table[w] for w in TYPES]).astype(np.float32)

    def text_feats(in_text, clip_model=None, clip_feat_dim=None, batch_size=64):
        if isinstance(in_text, str):
            in_text = [in_text]
        return np.stack([table[w] for w in in_text]).astype(np.float32)

    G.get_text_feats_multiple_templates = text_feats
    R.get_text_feats_multiple_templates = text_feats
    for attempt in range(1000):
        rooms = make_rooms(rng, T)
        if margins_ok(rooms, T):
            break
    else:
        raise SystemExit("no draw met the margins")
    reps = []
    orig = R.feats_denoise_dbscan

    def recording(feats, *a, **k):
        out = orig(feats, *a, **k)
        reps.append(np.asarray(out).reshape(-1).copy())
        return out

    R.feats_denoise_dbscan = recording
    ns = types.SimpleNamespace
    out = dict(types=np.array(TYPES), type_feats=T, words=np.array(words), table=np.stack([table[w] for w in words]),
               room_off=np.cumsum([0] + [len(o) for o, _ in rooms]), view_off=np.cumsum([0] + [len(v) for _, v in rooms]),
               emb64=np.concatenate([o for o, _ in rooms]).astype(np.float64),
               emb32=np.concatenate([o for o, _ in rooms]).astype(np.float32),
               view64=np.concatenate([v for _, v in rooms]).astype(np.float64))
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        g = G.Graph.__new__(G.Graph)
        g.clip_model, g.clip_feat_dim = "text table", D      # (generate_room_names asserts a model; the table above answers)
        g.rooms, g.objects = [], []
        for r, (objs, views) in enumerate(rooms):
            room = R.Room("0_%d" % r, "0", name="room%d" % r)
            room.embeddings = [v for v in views]
            for i, e in enumerate(objs.astype(dt)):
                ob = ns(object_id="0_%d_%d" % (r, i), room_id=room.room_id, embedding=e, name="thing")
                room.objects.append(ob)
                g.objects.append(ob)
            g.rooms.append(room)
        g.floors = [ns(floor_id="0", floor_zero_level=0.0, rooms=g.rooms)]
        reps.clear()
        g.generate_room_names(generate_method="obj_embedding", default_room_types=TYPES)
        out["ref_rep" + tag] = np.stack(reps).astype(dt)
        out["ref_names" + tag] = np.array([r.name for r in g.rooms])
        sc = np.sort(out["ref_rep" + tag].astype(np.float64) @ T.T.astype(np.float64), axis=1)
        assert np.all(sc[:, -1] - sc[:, -2] >= SCORE_MARGIN), "a representative's type scores are too close: change the seed"
        if tag == "64":
            # label-mode room query + the object query over its rooms (query_hierarchy_protected_icra's two stages)
            rl_all, oi_all, ri_all, sc_all = [], [], [], []
            for q, (room_q, obj_q) in enumerate([(TYPES[q % 3], "thing%d" % q) for q in range(6)]):
                rl = g.query_hmsg_room(room_q, floor_id=-1, query_method="label")
                oi, ri, sc = g.query_hmsg_object(obj_q, floor_id=-1, room_ids=rl, top_k=5, negative_prompt=["background"])
                pad = lambda a, n, v=-1: list(a) + [v] * (n - len(a))
                rl_all.append(pad(rl, len(rooms)))
                oi_all.append(pad(oi, 5))
                ri_all.append(pad(ri, 5))
                sc_all.append(pad(sc, 5, np.nan))
            out.update(ref_label_rooms=np.array(rl_all), ref_obj_idx=np.array(oi_all), ref_obj_room=np.array(ri_all),
                       ref_obj_score=np.array(sc_all, np.float64))
            g.generate_room_names(generate_method="view_embedding", default_room_types=TYPES)
            out["ref_view_names"] = np.array([r.name for r in g.rooms])
    assert out["ref_names64"][6] != out["ref_view_names"][6], "room 6 must name differently by objects and by views"
    out["meta"] = np.array(json.dumps(dict(eps=EPS, min_samples=2, dist_margin=DIST_MARGIN, score_margin=SCORE_MARGIN, attempts=attempt + 1)))
    path = os.path.join(REPO, "tests", "golden", "roomnames_obj.npz")
    np.savez_compressed(path, **out)
    print("roomnames_obj ok:", list(out["ref_names64"]), list(out["ref_view_names"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
