"""K1's workspace on the device: one grow-only buffer per (stream, table slots, table kind) shared by every point count, by the
single-cloud and the batch form, with `tables_clean` carried across sizes; bounded memory over a stream of varying clouds; a captured
chain that keeps replaying on its buffer while eager calls of other sizes use, outgrow and retire it."""
import numpy as np
import pytest
import torch

from oracle import cref
from tests.test_gpu_kernels import check_voxelize, dev

pytestmark = pytest.mark.gpu

R = [-4.0, -4.0, -3.0, 4.0, 4.0, 1.0]
V_DENSE = [0.4, 0.4, 4.0]           # 20 x 20 x 1 = 400 cells per agent: the per-cell table
V_HASH = [0.02, 0.02, 0.05]         # 400 x 400 x 80 cells, above 2^21: the hash grid, 2 x pow2ceil(n) slots


def _cloud(rng, n):
    return rng.uniform(-4.5, 4.5, (n, 4)).astype(np.float32)


@pytest.fixture
def vox(monkeypatch):
    """A side stream, this test's own workspace registry / clean set / retired list (the process-wide ones come back intact), and the
    (tables_clean, workspace identity) of every chain the test launches."""
    from heal_amd import _capi, derived, ops
    monkeypatch.setattr(ops, "_WS", {})
    monkeypatch.setattr(ops, "_VOX_CLEAN", set())
    monkeypatch.setattr(derived, "RETIRED", [])
    calls, real = [], _capi.call

    def recording(name, *args):
        if name in ("heal_voxelize", "heal_voxelize_batch"):
            calls.append((int(args[-2]), (args[-4].value, int(args[-3]))))      # ..., ws, ws_bytes, tables_clean, stream
        return real(name, *args)

    monkeypatch.setattr(_capi, "call", recording)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        yield st, calls
        st.synchronize()


def _entries():
    """{(table slots, dense): buffer} of the voxeliser's workspaces."""
    from heal_amd import ops
    return {k[0][1:]: b for k, b in ops._WS.items() if isinstance(k[0], tuple) and k[0][0] == "voxelize"}


def check_collated(clouds, voxel_size, P, max_voxels, got=None):
    from heal_amd import ops
    if got is None:
        got = ops.voxelize_collated([dev(c) for c in clouds], R, voxel_size, P, max_voxels)
    off = [int(v) for v in got[3].cpu()]
    assert off[0] == 0
    for b, cloud in enumerate(clouds):
        ov, oc, on = cref.voxelize(cloud, R, voxel_size, P, max_voxels, batch_idx=b)
        sl = slice(off[b], off[b + 1])
        assert off[b + 1] - off[b] == ov.shape[0]
        np.testing.assert_array_equal(got[0][sl].cpu().numpy().view(np.uint32), ov.view(np.uint32))
        np.testing.assert_array_equal(got[1][sl].cpu().numpy(), oc)
        np.testing.assert_array_equal(got[2][sl].cpu().numpy(), on)


@pytest.mark.parametrize("voxel_size", [V_DENSE, V_HASH], ids=["dense", "hash"])
def test_one_workspace_serves_every_size_in_any_order(vox, voxel_size):
    from heal_amd import derived
    _, calls = vox
    rng = np.random.default_rng(7)
    sizes = (4097, 63, 2049, 1, 2048, 4097, 65)
    for n in sizes:
        check_voxelize(_cloud(rng, n), R, voxel_size, 4, 50)
    check_voxelize(_cloud(rng, 3000), R, voxel_size, 80, 50)            # the max_points > 64 chain, on the same buffer
    check_collated([_cloud(rng, 1500), _cloud(rng, 700)], voxel_size, 4, 50)
    check_collated([_cloud(rng, 300), _cloud(rng, 1900)], voxel_size, 4, 50)
    assert len(calls) == len(sizes) + 3
    # tables_clean is 0 exactly on the first call on a buffer: the first call on a table, and the first after a regrowth
    seen = set()
    for clean, ident in calls:
        assert clean == (1 if ident in seen else 0), calls
        seen.add(ident)
    entries = _entries()
    assert len(seen) == len(entries) + len(derived.RETIRED)
    if voxel_size is V_DENSE:
        # 400 cells for the single clouds, 2 x 400 for the pair; the first buffer (sized for 8192 points) is never outgrown
        assert sorted(entries) == [(400, True), (800, True)] and derived.RETIRED == []
        assert [c for c, _ in calls] == [0] + [1] * len(sizes) + [0, 1]
    else:
        tables = {max(1024, 2 * (1 << (n - 1).bit_length())) for n in sizes + (3000, 2200)}
        assert set(entries) == {(t, False) for t in tables}
        assert [c for c, _ in calls[:len(sizes)]] == [0, 0, 0, 1, 0, 1, 1]


def test_memory_stays_bounded_over_varying_clouds(vox):
    """What ADVICE r6 asked for: clouds of ever-changing size neither add buffers nor leak; growth retires at most one buffer per
    doubling of the point count."""
    from heal_amd import derived, ops
    st, calls = vox
    rng = np.random.default_rng(11)
    base = _cloud(rng, 20_000)
    base_dev = dev(base)

    def run(n, check=False):
        cut = n // 3                                # two agents, adjacent slices of one buffer: read in place
        got = ops.voxelize_collated([base_dev[:cut], base_dev[cut:n]], R, V_DENSE, 32, 1000)
        if check:
            check_collated([base[:cut], base[cut:n]], V_DENSE, 32, 1000, got=got)
        del got
        st.synchronize()
        return torch.cuda.memory_allocated()

    mem = [run(int(n), check=(i == 39)) for i, n in enumerate(rng.integers(2050, 4097, 40))]
    assert mem[1] == mem[-1] and derived.RETIRED == [] and list(_entries()) == [(800, True)]
    assert [c for c, _ in calls] == [0] + [1] * 39
    del calls[:]
    mem = [run(int(n), check=(i == 39)) for i, n in enumerate(rng.integers(100, 20_001, 40))]
    assert list(_entries()) == [(800, True)]
    assert len(derived.RETIRED) <= 5                # capacities 1024 .. 32 768
    assert sum(1 for c, _ in calls if c == 0) == len(derived.RETIRED)


def test_replay_survives_eager_calls_of_other_sizes(vox):
    """A chain captured with tables_clean = 1 keeps replaying correctly while eager calls on the same stream use its buffer at a
    smaller size, then outgrow it (the old buffer is retired, still clean, and still the graph's)."""
    from heal_amd import derived, ops
    st, calls = vox
    rng = np.random.default_rng(13)
    a = _cloud(rng, 3000)
    a_dev = dev(a)
    clouds, clouds_dev = [a[:1100], a[1100:]], [a_dev[:1100], a_dev[1100:]]
    check_collated(clouds, V_DENSE, 32, 1000, got=ops.voxelize_collated(clouds_dev, R, V_DENSE, 32, 1000))   # eager warm-up
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        got = ops.voxelize_collated(clouds_dev, R, V_DENSE, 32, 1000)
    assert [c for c, _ in calls] == [0, 1]
    captured_ws = calls[-1][1]

    def replay_and_check():
        for t in got:
            t.fill_(-1)
        graph.replay()
        st.synchronize()
        check_collated(clouds, V_DENSE, 32, 1000, got=got)

    replay_and_check()
    check_collated([_cloud(rng, 200), _cloud(rng, 301)], V_DENSE, 32, 1000)          # smaller, same buffer
    assert calls[-1] == (1, captured_ws) and derived.RETIRED == []
    replay_and_check()
    check_collated([_cloud(rng, 2500), _cloud(rng, 2501)], V_DENSE, 32, 1000)        # above the capacity of 4096: regrown
    assert calls[-1][0] == 0 and calls[-1][1] != captured_ws
    assert [(b.data_ptr(), b.numel()) for b in derived.RETIRED] == [captured_ws]
    replay_and_check()
    check_collated([_cloud(rng, 2500), _cloud(rng, 2501)], V_DENSE, 32, 1000)
    assert calls[-1][0] == 1
    replay_and_check()
    del graph
