"""Record what the REFERENCE's box_alignment_relative_sample_np builds for the scenes of tests/posegraph_refs.golden_cases():

    python -m tests.golden.gen_pose_graph_golden        # needs the reference tree; writes tests/golden/pose_graph.npz

The reference optimises with g2o, which is not installed.  A recording stand-in for the `g2o` module (written here) is injected
into sys.modules before the reference is imported: its optimiser stores every add_vertex / add_edge call -- ids, fixed flag,
estimate, measurement, information -- and leaves the poses unchanged.  Only that recorded data and the scenes' inputs are
committed; the graph CONSTRUCTION is thereby pinned to the reference exactly, the minimiser is tested elsewhere.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pose_graph.npz")
RECORD = {"vertices": [], "edges": []}


class _SE2:
    def __init__(self, *a):
        v = np.asarray(a[0] if len(a) == 1 else a, dtype=np.float64).reshape(3)
        self._v = v.copy()

    def vector(self):
        return self._v.copy()


class _Vertex:
    kind = "SE2"

    def set_estimate(self, e):
        self.e = e

    def set_id(self, i):
        self.i = int(i)

    def set_fixed(self, f):
        self.f = bool(f)

    def estimate(self):
        return self.e


class _VertexXY(_Vertex):
    kind = "XY"


class _Edge:
    kind = "SE2"

    def __init__(self):
        self.v = {}

    def set_vertex(self, k, v):
        self.v[k] = v

    def set_measurement(self, m):
        self.m = m

    def set_information(self, info):
        self.info = np.array(info, dtype=np.float64)

    def set_robust_kernel(self, k):
        raise NotImplementedError


class _EdgeXY(_Edge):
    kind = "XY"


class _SparseOptimizer:
    def __init__(self):
        self._v = {}

    def set_algorithm(self, a):
        pass

    def set_verbose(self, v):
        pass

    def initialize_optimization(self):
        pass

    def optimize(self, n):
        RECORD["max_iterations"] = int(n)

    def vertex(self, i):
        return self._v[int(i)]

    def add_vertex(self, v):
        self._v[v.i] = v
        est = v.e.vector() if hasattr(v.e, "vector") else np.asarray(v.e, dtype=np.float64)
        RECORD["vertices"].append((v.i, v.f, v.kind == "SE2", np.asarray(est, dtype=np.float64)))

    def add_edge(self, e):
        m = e.m.vector() if hasattr(e.m, "vector") else np.asarray(e.m, dtype=np.float64)
        RECORD["edges"].append((e.v[0].i, e.v[1].i, e.kind == "SE2", np.asarray(m, dtype=np.float64), e.info))


def install_g2o():
    g = types.ModuleType("g2o")
    g.SE2, g.SparseOptimizer = _SE2, _SparseOptimizer
    g.VertexSE2, g.VertexPointXY, g.EdgeSE2, g.EdgeSE2PointXY = _Vertex, _VertexXY, _Edge, _EdgeXY
    for name in ("BlockSolverSE2", "LinearSolverDenseSE2", "LinearSolverCholmodSE2", "OptimizationAlgorithmLevenberg",
                 "BlockSolverSE3", "LinearSolverCholmodSE3"):
        setattr(g, name, lambda *a, **k: None)
    sys.modules["g2o"] = g


def record(ref_fn, s):
    """Run the reference on scene s -> dict of arrays (inputs, recorded graph, returned poses)."""
    from tests.posegraph_refs import OPTION_DEFAULTS
    RECORD["vertices"], RECORD["edges"] = [], []
    pose = s["pose"].copy()
    out = ref_fn([c.copy() for c in s["corners"]], pose, None if s["unc"] is None else [u.copy() for u in s["unc"]],
                 **{**OPTION_DEFAULTS, **s["opts"]})
    assert np.array_equal(pose, s["pose"]), "the reference changed noisy_lidar_pose in place"
    V, E = RECORD["vertices"], RECORD["edges"]
    vest = np.full((len(V), 3), np.nan)
    for k, v in enumerate(V):
        vest[k, :len(v[3])] = v[3]
    emeas, einfo = np.full((len(E), 3), np.nan), np.full((len(E), 3, 3), np.nan)
    for k, e in enumerate(E):
        emeas[k, :len(e[3])] = e[3]
        einfo[k, :e[4].shape[0], :e[4].shape[1]] = e[4]
    counts = np.array([len(c) for c in s["corners"]], dtype=np.int64)
    d = {"corners": np.concatenate([c.reshape(-1, 8, 3) for c in s["corners"]]), "counts": counts, "pose": s["pose"],
         "opts": np.array(json.dumps(s["opts"], sort_keys=True)), "has_unc": np.array(s["unc"] is not None),
         "unc": np.concatenate(s["unc"]) if s["unc"] is not None else np.zeros((0, 3)),
         "vid": np.array([v[0] for v in V], dtype=np.int64), "vfixed": np.array([v[1] for v in V], dtype=bool),
         "vse2": np.array([v[2] for v in V], dtype=bool), "vest": vest,
         "eij": np.array([[e[0], e[1]] for e in E], dtype=np.int64).reshape(-1, 2), "ese2": np.array([e[2] for e in E], dtype=bool),
         "emeas": emeas, "einfo": einfo, "returned": np.asarray(out, dtype=np.float64)}
    return d


def main():
    from tests.golden import ref_import
    from tests import posegraph_refs
    ref_import.install()
    install_g2o()
    import importlib
    ref = importlib.import_module("opencood.models.sub_modules.box_align_v2")
    blob = {}
    names = []
    for name, s in posegraph_refs.golden_cases().items():
        for k, v in record(ref.box_alignment_relative_sample_np, s).items():
            blob[f"{name}/{k}"] = v
        names.append(name)
        print(name, "vertices", len(blob[f"{name}/vid"]), "edges", len(blob[f"{name}/eij"]))
    blob["names"] = np.array(names)
    np.savez_compressed(OUT, **blob)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
