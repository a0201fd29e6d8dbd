"""The one pack cache (drone-yolo_amd/nn/modules/packs.py) on the CPU: every module-level pack accessor gives the bytes recorded in
tests/golden/pack_sites.json (tools/make_pack_sites_golden.py wrote it on the commit BEFORE the caches were unified, and says what the sites
and variants are), and every site follows the one staleness rule.  No GPU; needs the built library, like tests/test_pack_host.py."""
import copy
import importlib.util
import os

import pytest
import torch

from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.nn.modules.packs import PACKED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_pack_sites_golden", os.path.join(ROOT, "tools", "make_pack_sites_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

F16, BF16 = torch.float16, torch.bfloat16
# every site but the one whose record is that it declines (scale n's layers 0 / 1 are not the shape dy_stem2_fused is built for: there is no pack to keep)
RULE_SITES = [s for s in G.SITES if s != "model_n.stem2"]
PACK_TYPES = (H.PackedConv, H.PackedStem, H.PackedStem2, H.PackedC2f, H.PackedC2fTail, H.PackedC2fFront)


def fresh(site, root):
    """A deep copy of ``root`` that holds no pack: what it packs is what its weights say."""
    twin = copy.deepcopy(root)
    for m in twin.modules():
        m.__dict__.pop(PACKED, None)
    return twin


def get(site, root, dtype=F16, scaled=False):
    return G.get_variant(site, root, dtype, scaled)


def same(a, b) -> bool:
    """One pack object (``_packed_first`` hands back a new (pack, cout) tuple per call: its elements are compared)."""
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
        return all(x is y for x, y in zip(a, b))
    return a is b


def fold_tensors(site, root):
    """(name, tensor) of everything the site's fold reads: the floating parameters and buffers of its source modules."""
    return [(f"{i}.{n}", t) for i, m in enumerate(site.sources(root)) for n, t in list(m.named_parameters()) + list(m.named_buffers()) if t.is_floating_point()]


def test_every_site_packs_the_parents_bytes():
    table = G.load_table()
    assert sorted(table) == sorted(G.SITES) and sum(len(v) for v in table.values()) >= 200
    assert sum(1 for v in table.values() for d in v.values() if len(d) == 64) >= 120  # (most variants are packs, not refusals)
    for name in G.SITES:
        got = G.run_site(name)
        wrong = {v: (table[name].get(v), got.get(v)) for v in sorted(set(table[name]) | set(got)) if table[name].get(v) != got.get(v)}
        assert not wrong, f"{name}: (recorded, now) {wrong}"


@pytest.mark.parametrize("name", RULE_SITES)
def test_two_calls_return_one_pack_and_every_fold_tensor_is_watched(name):
    site = G.SITES[name]()
    root = site.root
    p0 = get(site, root)
    assert p0 is not None and same(get(site, root), p0)
    tensors = fold_tensors(site, root)
    assert len(tensors) >= 2
    for tname, t in tensors:
        for how in ("in place", "data replaced"):
            before = get(site, root)
            with torch.no_grad():
                if how == "in place":
                    t.add_(0.125)
                else:
                    t.data = t.data * 0.5 + 0.25
            after = get(site, root)
            assert not same(after, before), f"{name}: {tname} edited ({how}) and the old pack came back"
            assert same(get(site, root), after)
            assert G.digest(after) == G.digest(get(site, fresh(site, root))), f"{name}: after {tname} was edited ({how}) the pack is not what the weights say"
            assert G.digest(after) != G.digest(before), f"{name}: {tname} does not reach the pack (the edit should change its bytes)"


@pytest.mark.parametrize("name", RULE_SITES)
def test_owner_hooks_drop_what_version_counters_cannot_see(name):
    site = G.SITES[name]()
    root, owner = site.root, site.owner(site.root)
    p0 = get(site, root)
    owner.train()
    owner.eval()
    p1 = get(site, root)
    assert not same(p1, p0), "train() / eval() on the owner alone kept the pack"
    owner.load_state_dict(owner.state_dict())
    p2 = get(site, root)
    assert not same(p2, p1), "load_state_dict on the owner kept the pack"
    owner.to("cpu")  # already there: nothing moved
    assert same(get(site, root), p2), "a no-op move dropped the pack"
    owner.double()
    owner.float()  # a real cast (and back): new storage
    p3 = get(site, root)
    assert not same(p3, p2) and G.digest(p3) == G.digest(p2)


@pytest.mark.parametrize("name", RULE_SITES)
def test_a_slot_keeps_its_variants(name):
    site = G.SITES[name]()
    root = site.root
    a, b = get(site, root, F16), get(site, root, BF16)
    assert a is not None and b is not None and not same(a, b)
    assert same(get(site, root, F16), a) and same(get(site, root, BF16), b)
    on, off = get(site, root, F16, scaled=True), get(site, root, F16, scaled=False)
    assert same(off, a) and not same(on, a)
    assert same(get(site, root, F16, scaled=True), on)
    if site.layer0:  # ``_raw_input`` changes the fold, so it is part of the key: set, cleared and set again
        raw = G.get_variant(site, root, F16, True, raw=True)
        assert same(G.get_variant(site, root, F16, True, raw=False), on) and same(G.get_variant(site, root, F16, True, raw=True), raw)
        assert G.digest(raw) == G.digest(G.get_variant(site, fresh(site, root), F16, True, raw=True))


@pytest.mark.parametrize("name", RULE_SITES)
def test_fp8_activation_scale_repacks_the_fp8_variants_only(name):
    site = G.SITES[name]()
    root = site.root
    H.set_fp8_act_scale(G.FP8_ACT_SCALE)
    try:
        try:
            p8 = get(site, root, H.FP8)
        except (NotImplementedError, ValueError):
            p8 = None  # the site is not built for fp8 storage: the 16-bit pack must still not care about the scale
        p16 = get(site, root, F16)
        H.set_fp8_act_scale(2 * G.FP8_ACT_SCALE)
        assert same(get(site, root, F16), p16)
        if p8 is not None:
            q8 = get(site, root, H.FP8)
            assert not same(q8, p8)
            assert G.digest(q8) != G.digest(p8) or not isinstance(p8, H.PackedConv)  # (a PackedConv bakes the scale in; the stem rows and the 1x1 fragments do not)
            H.set_fp8_act_scale(G.FP8_ACT_SCALE)
            assert same(get(site, root, H.FP8), p8)
    finally:
        H.set_fp8_act_scale(1.0)
    assert name != "conv64" or p8 is not None  # (the plain convolution IS built for fp8: the branch above is not vacuous)


@pytest.mark.parametrize("name", RULE_SITES)
def test_a_filled_slot_puts_no_module_into_a_reference_cycle(name):
    """A module that keeps packs is still freed by reference counting (the parent commit's caches held no module either): one that had to
    wait for the garbage collector would take what its parameters' hooks hold — a trainer's captured graphs — into some later collection,
    possibly in the middle of another graph capture."""
    import gc
    import weakref

    site = G.SITES[name]()
    assert get(site, site.root) is not None and get(site, site.root, BF16, scaled=True) is not None
    refs = [weakref.ref(m) for m in site.root.modules() if not isinstance(m, torch.nn.SiLU)]  # (Conv.default_act is one shared instance)
    was = gc.isenabled()
    gc.disable()
    try:
        del site
        alive = [type(r()).__name__ for r in refs if r() is not None]
    finally:
        if was:
            gc.enable()
    assert not alive, f"{name}: still alive without a collection: {alive}"


def _holds_pack(obj, depth=4) -> bool:
    if isinstance(obj, PACK_TYPES):
        return True
    if depth and isinstance(obj, dict):
        return any(_holds_pack(v, depth - 1) for v in obj.values())
    if depth and isinstance(obj, (list, tuple)):
        return any(_holds_pack(v, depth - 1) for v in obj)
    return False


def _fill_some_slots(model):
    """Packs of every kind the model has, on the CPU; returns how many modules keep a store afterwards."""
    from drone_yolo_amd.nn.modules import C2f, Conv, Detect

    for m in model.modules():
        if isinstance(m, Conv):
            m._packed_for(torch.empty((1, max(m.conv.in_channels, 8), 1, 1), dtype=F16))
        if isinstance(m, C2f) and H.c2f_fused_supported(m.cv1.conv.in_channels, m.c, m.cv2.conv.out_channels, len(m.m), F16):
            m._packed_block(F16, "cpu")
        if isinstance(m, C2f) and m._tail_fusable(F16):
            m._packed_tail(F16, "cpu")
        if isinstance(m, Detect):
            m._packed_tail(F16, "cpu")
            m._packed_first(m.nl - 1, F16, "cpu")  # (None at scale n: 64 + 32 stacked channels are no multiple of 128)
    model.model[0]._packed_stem(F16, "cpu")
    return sum(1 for m in model.modules() if m.__dict__.get(PACKED))


def test_drop_packed_leaves_no_pack_anywhere():
    model = G.seeded(G.model("n"), "drop")
    assert _fill_some_slots(model) > 20
    assert any(_holds_pack(m.__dict__.get(PACKED)) for m in model.modules())
    epoch = model.weights_signature()[0]
    model.drop_packed()
    assert model.weights_signature()[0] == epoch + 1
    standard = set(torch.nn.Module().__dict__)
    for name, m in model.named_modules():
        assert not m.__dict__.get(PACKED), f"{name}: the store is not empty"
        left = [k for k, v in m.__dict__.items() if k not in standard and k != PACKED and _holds_pack(v)]
        assert not left, f"{name}: packs outside the store, under {left}"


def test_checkpoint_graph_carries_no_packs(tmp_path):
    from drone_yolo_amd.nn.checkpoint import read_checkpoint_dict, reference_module_graph, save_reference_checkpoint

    model = G.seeded(G.model("n"), "ckpt")
    _fill_some_slots(model)
    live = {id(m): m.__dict__[PACKED] for m in model.modules() if PACKED in m.__dict__}
    cp = reference_module_graph(model, model.state_dict())
    assert all(PACKED not in m.__dict__ and not _holds_pack(dict(m.__dict__)) for m in cp.modules())
    assert all(m.__dict__.get(PACKED) is live[id(m)] for m in model.modules() if id(m) in live) and len(live) > 20  # the live model keeps its packs
    path = tmp_path / "w.pt"
    save_reference_checkpoint(path, model, model.state_dict())
    ema = read_checkpoint_dict(str(path))["ema"]  # (the restricted unpickler would refuse a pack class outright)
    assert all(PACKED not in m.__dict__ for m in ema.modules())
    assert path.stat().st_size < 1.2 * 2 * sum(t.numel() for t in model.state_dict().values()) + (1 << 18)  # fp16 weights and the graph, nothing else
