"""The Detect decode of every path against float64, on logits that reach the decode row exactly (tests/_detect_util.py; the cases
are checked on the CPU by tests/test_detect_geometry_host.py):

    decode        detect_decode_kernel                   H.detect_decode, fp32 NHWC views wider than 64 + nc
    head_*        detect_head_kernel<f32 | bf16 | f16>,
                  detect_head_split_kernel               H.detect_head_decode behind S * identity / selector 1x1 weights
    hhead_*       conv3x3_hhead_kernel<bf16 | f16, 1|2>  H.detect_branch_fused behind a centre-tap identity 3x3 + SiLU and the same 1x1

Asserted per case: boxes (absolute) and scores (relative to max(score, 1e-7)) within 8 x the oracle's own fp32 error on the same
logits (``case_bars``); the candidate list at conf 0.25 and 0.001, with and without a class mask, against the float64 scores
outside the band conf (1 +- bar); the first arg-max on exact ties; keys built from the score written to ``pred``; counts; nothing
written outside the level's rows.  The users of detect_decode_row (decode, head_*) must agree bit for bit on the same logits.
Every test prints its measured errors beside the bars.
"""
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests import _detect_util as U

pytestmark = pytest.mark.gpu

SENT = -7777.0
GUARD = 256
HEAD_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "split": H.F16X2}


def nhwc(t, dtype, device, pad, fill):
    """CPU (N, C, H, W) float64 -> device NHWC view of ``dtype`` at pitch C + pad, the padding channels holding ``fill``."""
    n, c, h, w = t.shape
    buf = torch.full((n, h, w, c + pad), fill, dtype=dtype, device=device)
    buf[..., :c] = t.permute(0, 2, 3, 1).to(dtype).to(device)
    return buf.permute(0, 3, 1, 2)[:, :c]


def guarded(n, ch, A, device):
    buf = torch.full((2 * GUARD + n * ch * A,), SENT, dtype=torch.float32, device=device)
    return buf, buf[GUARD : GUARD + n * ch * A].view(n, ch, A)


def new_bufs(A, device):
    bufs = H.NmsBuffers(U.BATCH, A, 300, device)
    bufs.workspace.fill_(0xFF)
    return bufs


def collect(buf, pred, bufs, cols=None):
    """pred (CPU; its columns ``cols`` when the level rows sit inside a wider tensor) and, per image, the keys in ascending order;
    the class table.  Nothing outside the rows may have been written, and every image has ``counts`` keys."""
    torch.cuda.synchronize()
    flat = buf.cpu()
    assert bool((flat[:GUARD] == SENT).all()) and bool((flat[-GUARD:] == SENT).all()), "written outside pred"
    y = pred.cpu()
    if cols is not None:
        rest = torch.ones(y.shape[2], dtype=torch.bool)
        rest[cols] = False
        assert bool((y[:, :, rest] == SENT).all()), "written outside the level's anchors"
        y = y[:, :, cols]
    assert bool(torch.isfinite(y).all()) and not bool((y == SENT).any())
    res = dict(pred=y)
    if bufs is not None:
        counts, keys, cls = (t.cpu().numpy() for t in U.workspace_views(bufs))
        keys = keys.view(np.uint64)
        assert all(int((keys[b] != np.uint64(0xFFFFFFFFFFFFFFFF)).sum()) == counts[b] for b in range(U.BATCH)), "counts differ from the number of keys"
        res.update(keys=[np.sort(keys[b, : counts[b]]) for b in range(U.BATCH)], cls=cls.view(np.uint16))
    return res


# ---- the paths ----
def run_decode(case, device, conf=None, mask=None):
    nc = case.nc
    pad = (-(64 + nc)) % 4 + 4
    levels = [nhwc(f, torch.float32, device, pad, 50.0) for f in case.feats]  # (a padding channel read as a class would win every arg-max)
    buf, pred = guarded(U.BATCH, 4 + nc, case.anchors, device)
    bufs = new_bufs(case.anchors, device) if conf is not None else None
    H.detect_decode(levels, case.strides, nc, 16, out=pred, nms_bufs=bufs, conf_thres=conf or 0.0, classes_mask=mask)
    assert H.last_kernel_name().startswith("detect_decode_kernel"), H.last_kernel_name()
    return collect(buf, pred, bufs)


def c_cls_of(dt, nc):
    return 64 if nc <= 64 else (80 if dt == torch.float32 else 96)


@functools.lru_cache(maxsize=None)
def head_packs(tag, nc, device):
    dt = HEAD_DT[tag]
    src, bias = U.class_affine(nc)
    cc = c_cls_of(dt, nc)
    wc = torch.zeros(nc, cc)
    wc[torch.arange(nc), torch.from_numpy(src)] = U.S
    if cc > min(nc, 80):  # the last channel is fed zeros: a power of two there gives every row of the split pack another scale, and adds nothing
        wc[:, cc - 1] = 2.0 ** (torch.arange(nc) % 5)
    return (H.pack_frag1x1(torch.eye(64) * U.S, torch.full((64,), U.B0), dt, device), H.pack_frag1x1(wc, torch.from_numpy(bias).float(), dt, device))


def run_head(tag, case, device, conf=None, mask=None):
    dt, nc = HEAD_DT[tag], case.nc
    cc = c_cls_of(dt, nc)
    assert H.head_decode_supported(64, cc, nc, 16, dt), (tag, nc)
    xb, xc = [], []
    for x in case.x:
        n, _, h, w = x.shape
        cls_in = torch.full((n, cc, h, w), 20.0, dtype=torch.float64)  # channels no class reads: weight 0
        cls_in[:, : x.shape[1] - 64] = x[:, 64:]
        if cc > x.shape[1] - 64:
            cls_in[:, cc - 1] = 0.0  # (head_packs)
        if dt == H.F16X2:
            xb.append(H.to_nhwc(x[:, :64].float().contiguous().to(device), dt, c_pad=64))
            xc.append(H.to_nhwc(cls_in.float().to(device), dt, c_pad=cc))
        else:
            xb.append(nhwc(x[:, :64], dt, device, 16, 30.0))
            xc.append(nhwc(cls_in, dt, device, 16, 30.0))
    pb, pc = head_packs(tag, nc, device)
    buf, pred = guarded(U.BATCH, 4 + nc, case.anchors, device)
    bufs = new_bufs(case.anchors, device) if conf is not None else None
    n_lv = len(case.x)
    H.detect_head_decode(xb, xc, [pb] * n_lv, [pc] * n_lv, case.strides, nc, 16, out=pred, nms_bufs=bufs, conf_thres=conf or 0.0, classes_mask=mask)
    want = "detect_head_split_kernel" if dt == H.F16X2 else "detect_head_kernel"
    assert H.last_kernel_name().startswith(want), H.last_kernel_name()
    return collect(buf, pred, bufs)


@functools.lru_cache(maxsize=None)
def hhead_packs(dt, nc, device):
    w3 = torch.zeros(64, 64, 3, 3)
    w3[torch.arange(64), torch.arange(64), 1, 1] = 1.0
    pc3 = H.PackedConv(w3, torch.zeros(64), 1, 1, 1, True, dt, device)
    wc = torch.zeros(nc, 64)
    wc[torch.arange(nc), torch.arange(nc)] = U.S
    return pc3, H.pack_frag1x1(torch.eye(64) * U.S, torch.full((64,), U.B0), dt, device), H.pack_frag1x1(wc, torch.full((nc,), U.B0), dt, device)


def run_hhead(dt, case, device, conf=None, mask=None):
    """One call per level and branch into a pred with sentinel columns in front of, between and behind the levels."""
    nc = case.nc
    pc3, wbox, wcls = hhead_packs(dt, nc, device)
    a0, A = [], 5
    for h, w in case.shapes:
        a0.append(A)
        A += h * w + 3
    A += 4
    cols = torch.cat([torch.arange(a, a + h * w) for a, (h, w) in zip(a0, case.shapes)])
    buf, pred = guarded(U.BATCH, 4 + nc, A, device)
    bufs = new_bufs(A, device) if conf is not None else None
    if bufs is not None:
        H.nms_reset_counts(bufs)
    for x, s, a in zip(case.x, case.strides, a0):
        n, _, h, w = x.shape
        cls_in = torch.zeros((n, 64, h, w), dtype=torch.float64)
        cls_in[:, :nc] = x[:, 64:]
        H.detect_branch_fused(nhwc(x[:, :64], dt, device, 8, 40.0), pc3, wbox[0], wbox[1], 1, nc, 16, s, pred, a)
        assert H.last_kernel_name().startswith("conv3x3_hhead"), H.last_kernel_name()
        H.detect_branch_fused(nhwc(cls_in, dt, device, 8, 40.0), pc3, wcls[0], wcls[1], 2, nc, 16, s, pred, a, nms_bufs=bufs, conf_thres=conf or 0.0, classes_mask=mask)
        assert H.last_kernel_name().startswith("conv3x3_hhead"), H.last_kernel_name()
    res = collect(buf, pred, bufs, cols)
    if bufs is not None:  # anchors of the wide tensor -> anchors of the levels
        inv = np.full(A, -1, np.int64)
        inv[cols.numpy()] = np.arange(len(cols))
        for b in range(U.BATCH):
            a = inv[(res["keys"][b] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
            assert (a >= 0).all(), "a candidate outside the level's anchors"
            res["keys"][b] = (res["keys"][b] & np.uint64(0xFFFFFFFF00000000)) | a.astype(np.uint64)
        res["cls"] = res["cls"][:, cols.numpy()]
    return res


# ---- the checks ----
def check_values(path, case, cases, res):
    err, bar = U.errors(res["pred"], U.reference(case)), U.case_bars(case, cases)
    print(f"| {path} | {case.name} | " + " | ".join(f"{err[k]:.2e} / {bar[k]:.2e}" for k in ("xy", "wh", "sc")) + " |")
    for k in ("xy", "wh", "sc"):
        assert err[k] <= bar[k], f"{path} {case.name}: {k} error {err[k]:.3e} above the bar {bar[k]:.3e}"


def check_candidates(path, case, cases, res, conf, mask):
    m = U.case_bars(case, cases)["sc"]
    must, may_not, j, tied = U.expected_candidates(case, conf, mask, m)
    y = res["pred"].numpy()
    what = f"{path} {case.name} conf {conf} mask {mask is not None}"
    for b in range(U.BATCH):
        keys = res["keys"][b]
        a = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert len(np.unique(a)) == len(a) and (a < case.anchors).all(), what
        listed = np.zeros(case.anchors, bool)
        listed[a] = True
        assert not (must[b] & ~listed).any(), f"{what}: image {b} misses {int((must[b] & ~listed).sum())} candidates"
        assert not (may_not[b] & listed).any(), f"{what}: image {b} lists {int((may_not[b] & listed).sum())} anchors it may not"
        cls = res["cls"][b][a].astype(np.int64)
        assert (cls < case.nc).all(), what
        sure = must[b][a]
        assert (cls[sure] == j[b][a][sure]).all(), f"{what}: image {b}, class of {int((cls[sure] != j[b][a][sure]).sum())} candidates (of them exact ties: {int((tied[b][a][sure] & (cls[sure] != j[b][a][sure])).sum())})"
        score = y[b, 4 + cls, a]
        assert (score == y[b][4:, a].max(0)).all(), f"{what}: the stored class does not hold the best written score"
        want = ((~score.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | a.astype(np.uint64)
        assert np.array_equal(keys, want), f"{what}: keys are not (~score bits << 32) | anchor of the written score"


def by_nc(cases, nc):
    return [c for c in cases if c.nc == nc]


def sweep(path, run, cases, nc, device):
    """The cases of one nc; the bars' fallback looks at the whole sweep."""
    for case in by_nc(cases, nc):
        first = None
        for conf in U.CONFS:
            for mask in (None, U.class_mask(case.nc).to(device)):
                res = run(case, device, conf, mask)
                if first is None:
                    first = res
                    check_values(path, case, cases, res)
                else:
                    assert torch.equal(res["pred"], first["pred"]), f"{path} {case.name}: the filter's arguments change pred"
                check_candidates(path, case, cases, res, conf, None if mask is None else mask.cpu())


@pytest.mark.parametrize("nc", [80, 3])
def test_decode_kernel(nc, device):
    sweep("decode", run_decode, U.decode_cases(), nc, device)


@pytest.mark.parametrize("nc", [10, 1, 40, 80, 128])
@pytest.mark.parametrize("tag", list(HEAD_DT))
def test_head_kernels(tag, nc, device):
    sweep(f"head_{tag}", functools.partial(run_head, tag), U.head_cases(), nc, device)


@pytest.mark.parametrize("nc", [10, 1, 40, 80, 128])
def test_users_of_the_shared_row_agree_bit_for_bit(nc, device):
    for case in by_nc(U.head_cases(), nc):
        want = run_decode(case, device)["pred"]
        for tag in HEAD_DT:
            got = run_head(tag, case, device)["pred"]
            assert torch.equal(got, want), f"head_{tag} {case.name}: {int((got != want).sum())} values differ from detect_decode_kernel's"


@pytest.mark.parametrize("nc", [10, 1, 16])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_hhead_branches(dt, nc, device):
    tag = "bf16" if dt == torch.bfloat16 else "f16"
    sweep(f"hhead_{tag}", functools.partial(run_hhead, dt), U.hhead_cases(), nc, device)
