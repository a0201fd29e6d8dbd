"""Writes (or, with --check, compares against) tests/golden/pack_sites.json: what every MODULE-level weight-pack accessor of the
inference path hands its kernel, per site and variant one SHA-256 over every tensor the pack holds plus its scalar fields.

    python tools/make_pack_sites_golden.py            # record
    python tools/make_pack_sites_golden.py --check    # compare; exit status 1 on any difference

tools/make_pack_golden.py pins the packers (``PackedConv`` ... on given weights); this one pins what the modules feed them: the BatchNorm
fold, the activation-domain fold, the stacking and the arguments.  Needs the built library, no GPU.  Only the accessors are called
(``_packed_for``, ``_packed_stem``, ``_packed_cv3``, ``_packed_block``, ``_packed_tail``, ``_packed_front``, ``_packed_first``,
``_stem2_pack``), so the script runs on any commit that has them: a refactor of the pack caches is right when --check reports no
difference before and after it.  (``_packed_stem`` is younger than the file: on a commit without it ``Conv.forward_stem``'s inline pack
is restated here.)

A site is a seeded CPU module tree (``SITES[name]()`` -> ``Site``): ``root`` holds every module the pack reads (so ``copy.deepcopy(root)``
is a fresh, cache-free twin), ``get(root, dtype)`` calls the accessor, ``owner(root)`` is the module that keeps the pack, ``sources(root)``
the modules whose parameters and buffers the fold reads.  Variants: five storage types x the log2(e)-scaled activation domain off / on
(x ``_raw_input`` off / on for the sites that can be layer 0); a site that refuses a storage type is recorded as "raises:<exception>", one
that declines (returns None) as "none".  tests/test_pack_cache_host.py replays the file and checks the staleness rule on the same sites.
"""
from __future__ import annotations

import argparse
import copy
import hashlib
import json
import sys
import zlib
from pathlib import Path
from typing import Callable, NamedTuple

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import drone_yolo_amd as D  # noqa: E402
from drone_yolo_amd import hip_ops as H  # noqa: E402
from drone_yolo_amd.nn.modules.block import C2f, Proto, RepVGGBlock  # noqa: E402
from drone_yolo_amd.nn.modules.conv import Conv, DWConv, PlainConv2d, fold_conv_bn  # noqa: E402
from drone_yolo_amd.nn.modules.head import Detect  # noqa: E402

TABLE = ROOT / "tests" / "golden" / "pack_sites.json"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "fp8": H.FP8, "x2": H.F16X2}
FP8_ACT_SCALE = 0.05
CPU = torch.device("cpu")


class Site(NamedTuple):
    root: nn.Module
    get: Callable  # (root, dtype) -> the pack (any nesting of pack objects, tensors, tuples and scalars) or None
    owner: Callable  # root -> the module that keeps the pack
    sources: Callable  # root -> the modules whose parameters and buffers the fold reads
    layer0: bool = False  # can be the layer that reads the image: recorded with ``_raw_input`` set as well


class LegacyDetect(Detect):
    legacy = True  # the v8 YAMLs' class branch (two 3x3 convolutions), as ``parse_model`` builds it


def seeded(m: nn.Module, name: str) -> nn.Module:
    """``m`` in eval mode with every parameter and BatchNorm statistic drawn from a generator seeded by ``name``."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    for p in m.parameters():
        p.data = torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.3) + (1.0 if p.dim() == 1 else 0.0)
    for b in m.modules():
        if isinstance(b, nn.BatchNorm2d):
            b.running_mean.copy_(torch.randn(b.running_mean.shape, generator=g) * 0.1)
            b.running_var.copy_(torch.rand(b.running_var.shape, generator=g) + 0.5)
            b.eps = 1e-3
    return m.eval()


def _x(c: int, dtype) -> torch.Tensor:
    """What ``_packed_for`` reads of its input: dtype, device and channel count."""
    return torch.empty((1, c, 1, 1), dtype=dtype)


def _self(r):
    return r


def _own(r):
    return (r,)


def _for(cin: int):
    return lambda r, dt: r._packed_for(_x(cin, dt))


def _stem_pack(conv, dtype):
    if hasattr(conv, "_packed_stem"):
        return conv._packed_stem(dtype, CPU)
    w, b = fold_conv_bn(conv.conv.weight, conv.conv.bias, conv.bn)  # (a commit before ``_packed_stem``: Conv.forward_stem's inline pack)
    w, b, act = H.domain_fold(w, b, isinstance(conv.act, nn.SiLU), raw_input=True)
    return H.PackedStem(w, b, act, dtype, CPU)


def model(scale: str = "n"):
    import yaml

    d = yaml.safe_load(open(ROOT / "drone-yolo_amd" / "cfg" / "models" / "v8" / "yolov8-p2-repvgg.yaml"))
    d["scale"], d["nc"] = scale, 10
    return D.DetectionModel(dict(d), nc=10, verbose=False)


def _stem2(model, dtype):
    if not hasattr(model, "_place"):
        model._plan_graph()
    return model._stem2_pack(torch.empty((1, 3, 64, 64)), dtype, consumers0=model._consumers0)


def _site(name, module, get, owner=_self, sources=_own, layer0=False):
    return name, lambda: Site(seeded(module(), name), get, owner, sources, layer0)


SITES = dict([
    _site("conv64", lambda: Conv(64, 64, 3), _for(64)),
    _site("conv_image.stem", lambda: Conv(3, 32, 3, 2), _stem_pack, layer0=True),
    _site("conv_image.padded", lambda: Conv(3, 32, 3, 2), lambda r, dt: r._packed_for(_x(H.chan_gran(dt), dt)), layer0=True),
    _site("dwconv", lambda: DWConv(64, 128, 3), _for(64)),
    _site("repvgg", lambda: RepVGGBlock(64, 64), _for(64), layer0=True),
    _site("repvgg_s2", lambda: RepVGGBlock(64, 128, stride=2), _for(64)),
    _site("plain1x1", lambda: PlainConv2d(64, 64, 1), _for(64)),
    _site("proto.upsample", lambda: Proto(64, 64, 32), _for(64), sources=lambda r: (r.upsample,)),
    _site("proto.cv3", lambda: Proto(64, 64, 32), lambda r, dt: r._packed_cv3(_x(64, dt)), sources=lambda r: (r.cv3,)),
    _site("c2f.block", lambda: C2f(64, 64, 1, True), lambda r, dt: r._packed_block(dt, CPU), sources=lambda r: (r.cv1, r.m[0].cv1, r.m[0].cv2, r.cv2)),
    _site("c2f.tail_n1", lambda: C2f(128, 128, 1, False), lambda r, dt: r._packed_tail(dt, CPU), sources=lambda r: (r.m[-1].cv2, r.cv2)),
    _site("c2f.tail_n2", lambda: C2f(128, 128, 2, True), lambda r, dt: r._packed_tail(dt, CPU), sources=lambda r: (r.m[-1].cv2, r.cv2)),
    _site("c2f.front", lambda: nn.ModuleList([Conv(64, 128, 3, 2), C2f(128, 128, 1)]), lambda r, dt: r[1]._packed_front(r[0], dt, CPU),
          owner=lambda r: r[1], sources=lambda r: (r[0], r[1].cv1)),
    _site("detect.tail", lambda: LegacyDetect(10, (64, 128)), lambda r, dt: r._packed_tail(dt, CPU),
          sources=lambda r: [s[-1] for s in r.cv2] + [s[-1] for s in r.cv3]),
    _site("detect.first0", lambda: LegacyDetect(10, (64, 128)), lambda r, dt: r._packed_first(0, dt, CPU), sources=lambda r: (r.cv2[0][0], r.cv3[0][0])),
    _site("detect.first1", lambda: LegacyDetect(10, (64, 128)), lambda r, dt: r._packed_first(1, dt, CPU), sources=lambda r: (r.cv2[1][0], r.cv3[1][0])),
    # scale n opens Conv(3, 16) -> RepVGGBlock(16, 32): dy_stem2_fused is built for 32 -> 64 (scale s), so n records that the site declines
    _site("model_n.stem2", model, _stem2, sources=lambda r: (r.model[0], r.model[1]), layer0=True),
    _site("model_s.stem2", lambda: model("s"), _stem2, sources=lambda r: (r.model[0], r.model[1]), layer0=True),
])


def _feed(h, obj) -> None:
    if isinstance(obj, torch.Tensor):
        h.update(f"T{obj.dtype}{tuple(obj.shape)}".encode())
        h.update(obj.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    elif isinstance(obj, (list, tuple)):
        h.update(b"[")
        for o in obj:
            _feed(h, o)
        h.update(b"]")
    elif obj is None or isinstance(obj, (bool, int, float, str, torch.dtype)):
        h.update(repr(obj).encode() + b";")
    else:  # a pack object: its public fields by name (the private ones hold sources and lazily built twins)
        for k in sorted(vars(obj)):
            if not k.startswith("_"):
                h.update(k.encode() + b"=")
                _feed(h, vars(obj)[k])


def digest(pack) -> str:
    """SHA-256 over every tensor (dtype, shape, bytes) and scalar field the pack holds; "none" for a site that declined."""
    if pack is None:
        return "none"
    h = hashlib.sha256()
    _feed(h, pack)
    return h.hexdigest()


def variants(site: Site):
    """(name, dtype, scaled domain, _raw_input) of every variant the site is recorded in."""
    return [(f"{dt}|{'l2e' if scaled else 'ref'}{'|raw' if raw else ''}", DTYPES[dt], scaled, raw)
            for dt in DTYPES for scaled in (False, True) for raw in ((False, True) if site.layer0 else (False,))]


def set_raw_input(site: Site, root, raw: bool) -> None:
    """What the model executor does to the layer that reads the image (nn/tasks.py::_scaled_domain_for)."""
    first = site.sources(root)[0]
    if raw:
        first._raw_input = True
    else:
        first.__dict__.pop("_raw_input", None)


def get_variant(site: Site, root, dtype, scaled: bool, raw: bool = False):
    """The site's pack for one variant (the fp8 activation scale is whatever is in force)."""
    set_raw_input(site, root, raw)
    with H.scaled_activations(scaled):
        return site.get(root, dtype)


def run_site(name: str) -> dict:
    site = SITES[name]()
    out = {}
    H.set_fp8_act_scale(FP8_ACT_SCALE)
    try:
        for vname, dtype, scaled, raw in variants(site):
            try:
                # (a fresh twin per variant: the record is what a cache-free module packs, whatever the commit's caches key on)
                out[vname] = digest(get_variant(site, copy.deepcopy(site.root), dtype, scaled, raw))
            except (NotImplementedError, ValueError, TypeError, RuntimeError) as e:
                out[vname] = f"raises:{type(e).__name__}"
    finally:
        H.set_fp8_act_scale(1.0)
    return out


def load_table(path=TABLE) -> dict:
    with open(path) as f:
        return json.load(f)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare against the committed file instead of writing it")
    ap.add_argument("--table", default=str(TABLE))
    a = ap.parse_args()
    got = {name: run_site(name) for name in SITES}
    n = sum(len(v) for v in got.values())
    if not a.check:
        with open(a.table, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(got)} sites, {n} variants to {a.table}")
        return 0
    want = load_table(a.table)
    diff = [(s, v) for s in sorted(set(want) | set(got)) for v in sorted(set(want.get(s, {})) | set(got.get(s, {})))
            if want.get(s, {}).get(v) != got.get(s, {}).get(v)]
    for s, v in diff[:40]:
        print(f"DIFFERS {s} {v}\n  file {want.get(s, {}).get(v)}\n  now  {got.get(s, {}).get(v)}")
    print(f"{len(got)} sites, {n} variants, {len(diff)} differences against {a.table}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
