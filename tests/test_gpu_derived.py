"""heal_amd/derived.py on the device: a captured graph keeps reading the weight-derived tensors it was captured with after an
eager call replaced them, and a repeated eager step builds nothing new."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_replay_after_a_weight_change_reads_the_retired_folds():
    """Capture a BasicBlock (two Conv + BatchNorm folds), change the BatchNorm statistics in place, run the block eagerly (which
    replaces the folded entries), then hand the allocator's small blocks to new tensors full of other values: the replay must still
    return the captured output bit for bit, and (HEAL_GRAPH_GUARD=1) every address the capture logged must still be live."""
    from heal_amd import _capi
    from heal_amd.opencood.models.sub_modules.bev_blocks import BasicBlock
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    blk = BasicBlock(64, 64).to(dev).eval()
    for bn in (blk.bn1, blk.bn2):
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 64, 64, 64, device=dev)
    st = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(st):
        blk(x)                                            # eager: builds the folds and their fragment layouts
        _capi.guard_take()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            y = blk(x)
        log = _capi.guard_take()
        g.replay()
        st.synchronize()
        want = y.clone()
        for bn in (blk.bn1, blk.bn2):
            bn.running_var.mul_(2.0)
            bn.running_mean.add_(0.25)
        changed = blk(x)                                  # replaces the entries the graph reads
        sizes = {t.numel() for bn in (blk.bn1, blk.bn2) for t in (bn.weight, blk.conv1.weight)}
        junk = [torch.full((n,), 1e30, device=dev) for n in sorted(sizes) for _ in range(32)]
        _capi.guard_check(log, "replay after a weight change")
        g.replay()
        st.synchronize()
    assert not torch.equal(changed, want)
    assert torch.equal(y, want)
    del junk


def test_second_eager_step_builds_nothing(monkeypatch):
    """The 5-agent scene (bench.py scene5): a second identical eager step finds every derived tensor in the store, and the store
    holds less than half its bound (no eviction can thrash within a step)."""
    from heal_amd import configs, derived
    from heal_amd.pipeline import Scene, ScenePipeline
    monkeypatch.setattr(derived, "_STORE", type(derived._STORE)())   # this scene's entries only; the real store comes back intact
    mods = ["m1", "m1", "m1", "m2", "m4"]
    st = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(st):
        pipe = ScenePipeline(configs.heal_heter(tuple(sorted(set(mods))), max_cav=5), "cuda:0", seed=0)
        scene = Scene(len(mods), seed=4, device="cuda:0", modalities=mods)
        pipe.step(scene)
        built, live = derived.builds, derived.live()
        pipe.step(scene)
    torch.cuda.synchronize()
    print(f"derived entries after one scene5 step: {live}")
    assert derived.builds == built and derived.live() == live
    assert 0 < live < derived.BOUND // 2
