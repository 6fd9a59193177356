"""GPU parity: the HIP path (through the C-ABI of libdct_amd.so) against the
oracle and the reference's golden vectors.  Integer outputs must be bit-exact;
float outputs within 1e-4 (BASELINE.json north_star)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import f64

pytestmark = pytest.mark.gpu

QUALITIES = [1, 10, 25, 50, 75, 90, 100]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import dct_amd
    dct_amd.lib()
    return torch


@pytest.fixture(scope="module")
def dm(T):
    import dct_amd
    return dct_amd


def gpu_px(T, px):
    return T.from_numpy(np.ascontiguousarray(px)).cuda()


def test_synth_matches_oracle(T, dm):
    import oracle as O
    for kind, k in O.KINDS.items():
        for (w, h) in [(128, 128), (40, 24), (1920, 1080)]:
            g = dm.synth(777, kind, w, h).cpu().numpy()[0]
            assert np.array_equal(g, O.synth_plane(777, k, w, h)), (kind, w, h)


def test_forward_quant_tiles_bit_exact(T, dm, tiles):
    """128x128 tiles of every synthetic kind vs the REFERENCE's own quantized output."""
    for kind in ["uniform", "smooth", "const", "extreme"]:
        px = tiles[f"{kind}_px"]
        g = gpu_px(T, px)
        for q in QUALITIES:
            for ad in (0, 1):
                out = dm.Plan(q, ad).forward_quant(g).cpu().numpy()
                want = tiles[f"{kind}_q{q}_a{ad}"]
                bad = np.argwhere(out != want)
                assert bad.size == 0, f"{kind} q{q} a{ad}: {len(bad)} mismatches, first {bad[:4].tolist()}"


def test_forward_quant_full_size_digests(T, dm, digests):
    """BASELINE sizes (4K luma, 4K 4:2:0 chroma, 512^2): sha256 of the int16 planes
    equals the reference's, frames regenerated on the device from the seed."""
    seed = digests["seed"]
    for e in digests["entries"]:
        px = dm.synth(seed, e["kind"], e["width"], e["height"])
        out = dm.Plan(e["quality"], e["adaptive"]).forward_quant(px).cpu().numpy()
        got = hashlib.sha256(out.tobytes()).hexdigest()
        assert got == e["sha256"], e


@pytest.mark.parametrize("kind,q,ad,F", [("uniform", 50, 0, 64), ("smooth", 90, 1, 16), ("const", 75, 0, 16),
                                         ("extreme", 10, 1, 8), ("uniform", 100, 0, 8), ("extreme", 97, 0, 8)])
def test_bench_workload_every_block(T, dm, kind, q, ad, F):
    """The bench's own step (F 4K luma + 2F 1080p chroma planes in one dctq_forward_quant_planes launch;
    F = 64 is the headline 12 441 600 blocks with bench.py's seeds) checked block by block against the
    oracle -- the headline number's output, not a sample of it -- plus other input kinds, qualities (tie-heavy
    q97 / q100 included) and the adaptive mode at bench geometry.  Twice: as the bench launches it (no
    variance output: the kernel instantiation the bench times, with its 2-lane tie rounds) and with var_num,
    checked against the exact block variance numerator."""
    import oracle as O
    luma = dm.synth(12345, kind, 3840, 2160, F)
    chroma = dm.synth(12345 + 50000, kind, 1920, 1080, 2 * F)
    ny, nc = F * 480 * 270, 2 * F * 240 * 135
    vy = T.empty(ny, dtype=T.int32, device="cuda")
    vc = T.empty(nc, dtype=T.int32, device="cuda")
    plan = dm.Plan(q, ad)
    by, bc = plan.forward_quant_planes([luma, chroma])
    cy, cc = plan.forward_quant_planes([luma, chroma], var_nums=[vy, vc])
    threads = min(16, os.cpu_count() or 1)
    for px, bench_c, coef, vn, per in ((luma, by, cy, vy, 480 * 270), (chroma, bc, cc, vc, 240 * 135)):
        host_px = px.cpu().numpy()
        host_b = bench_c.cpu().numpy()
        host_c = coef.cpu().numpy()
        host_v = vn.cpu().numpy()
        for f in range(px.shape[0]):
            want = O.forward_plane(host_px[f], q, ad, threads)
            assert np.array_equal(host_b[f * per:(f + 1) * per], want), f"{kind}: frame {f} of {tuple(px.shape)}"
            assert np.array_equal(host_c[f * per:(f + 1) * per], want), f"{kind} +var: frame {f} of {tuple(px.shape)}"
        wv = O.plane_variance(host_px[-1]) * 4096.0  # var_num / 4096 == calculate_block_variance exactly
        assert np.array_equal(host_v[-per:].astype(np.float64), wv), kind


def test_forward_quant_vs_oracle_many_seeds(T, dm):
    import oracle as O
    rng = np.random.default_rng(5)
    for trial in range(12):
        kind = ["uniform", "smooth", "const", "extreme"][trial % 4]
        q = int(rng.integers(1, 101))
        ad = int(trial % 3 == 0)
        w, h = 8 * int(rng.integers(1, 90)), 8 * int(rng.integers(1, 40))
        px = O.synth_plane(1000 + trial, O.KINDS[kind], w, h)
        got = dm.Plan(q, ad).forward_quant(gpu_px(T, px)).cpu().numpy()
        want = O.forward_plane(px, q, ad)
        assert np.array_equal(got, want), (kind, q, ad, w, h, int((got != want).sum()))


def test_quality_sweep_adversarial(T, dm):
    """Every quality 1..100, both modes, on inputs built to hit rounding ties:
    constant blocks (DC = 8*(p-128)), two-level stripes and checkerboards."""
    import oracle as O
    rng = np.random.default_rng(11)
    blocks = []
    for v in range(256):
        blocks.append(np.full((8, 8), v, np.uint8))
    for _ in range(128):
        a, b = rng.integers(0, 256, 2)
        m = np.indices((8, 8)).sum(0) % 2 == 0
        blocks.append(np.where(m, a, b).astype(np.uint8))
        s = np.zeros((8, 8), np.uint8)
        s[:, :4], s[:, 4:] = a, b
        blocks.append(s)
        blocks.append(s.T.copy())
    blocks.append(np.zeros((8, 8), np.uint8))
    blocks.append(np.full((8, 8), 255, np.uint8))
    nb = len(blocks)
    px = np.concatenate(blocks, axis=1)  # one block row, nb blocks wide
    g = gpu_px(T, px)
    for q in range(1, 101):
        for ad in (0, 1):
            got = dm.Plan(q, ad).forward_quant(g).cpu().numpy()
            want = O.forward_plane(px, q, ad)
            assert np.array_equal(got, want), (q, ad, int((got != want).sum()))
    assert nb > 64


def test_edge_geometries(T, dm):
    """Block counts not multiple of the wave/workgroup size, single column/row,
    padded row stride, multi-frame stacks with a frame gap."""
    import torch
    import oracle as O
    for (w, h) in [(8, 8), (8, 64), (512, 8), (8 * 63, 8), (8 * 65, 8), (8 * 257, 8), (24, 16)]:
        px = O.synth_plane(3, 0, w, h)
        got = dm.Plan(50, 0).forward_quant(gpu_px(T, px)).cpu().numpy()
        assert np.array_equal(got, O.forward_plane(px, 50, 0)), (w, h)
    # padded stride + frame gap: [F, H, Wpad] buffer, view [:, :, :W]
    F, H, W, Wp = 3, 40, 56, 72
    big = torch.zeros((F, H + 2, Wp), dtype=torch.uint8, device="cuda")
    ref = []
    for f in range(F):
        p = O.synth_plane(40 + f, f % 4, W, H)
        big[f, :H, :W] = torch.from_numpy(p).cuda()
        ref.append(O.forward_plane(p, 75, 1))
    view = big[:, :H, :W]
    got = dm.Plan(75, 1).forward_quant(view).cpu().numpy()
    assert np.array_equal(got, np.concatenate(ref))


def test_var_num_exact(T, dm, tiles):
    import oracle as O
    for kind in ["uniform", "smooth", "const"]:
        px = tiles[f"{kind}_px"]
        vn = T.zeros(px.size // 64, dtype=T.int32, device="cuda")
        dm.Plan(50, 1).forward_quant(gpu_px(T, px), var_num=vn)
        var = vn.cpu().numpy().astype(np.float64) / 4096.0
        assert np.array_equal(var, O.plane_variance(px)), kind


def test_fallback_counter_and_exactness(T, dm):
    """Ties are resolved exactly, and the fallback counter sees the exact path run.

    * constant 8x8 blocks at q50: the DC is an exact .5 tie for half of them; the
      kernel resolves those from the plan's constant-block DC table, so the exact
      path never runs (counter 0) and the output is still the reference's;
    * left/right step blocks (a|b) at q50: DC/Q = (a+b)/4 - 64 ties whenever
      a+b = 2 mod 4 (a quarter of the blocks) and the blocks are not flat, so
      those DCs go through the exact fp64 path."""
    import oracle as O
    plan = dm.Plan(50, 0)
    cnt = T.zeros(1, dtype=T.int64, device="cuda")
    plan.set_fallback_counter(cnt)

    px = O.synth_plane(9, 2, 1024, 512)
    got = plan.forward_quant(gpu_px(T, px)).cpu().numpy()
    assert np.array_equal(got, O.forward_plane(px, 50, 0))
    assert int(cnt.item()) == 0

    rng = np.random.default_rng(5)
    by, bx = 64, 128
    ab = rng.integers(0, 256, (by, bx, 2), dtype=np.uint8)
    blk = np.concatenate([np.repeat(ab[:, :, :1, None], 4, 3).repeat(8, 2),
                          np.repeat(ab[:, :, 1:, None], 4, 3).repeat(8, 2)], axis=3)  # [by, bx, 8, 8]
    px = np.ascontiguousarray(blk.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8))
    got = plan.forward_quant(gpu_px(T, px)).cpu().numpy()
    plan.set_fallback_counter(None)
    assert np.array_equal(got, O.forward_plane(px, 50, 0))
    a, b = ab[:, :, 0].astype(int), ab[:, :, 1].astype(int)
    ties = int(((((a + b) % 4) == 2) & (a != b)).sum())  # a == b blocks are flat: table, not exact path
    n = int(cnt.item())
    assert ties <= n < ties + 0.05 * by * bx, (n, ties)


def _adversarial_row():
    """One block row of tie-prone blocks: every constant block, two-level checkerboards and stripes."""
    rng = np.random.default_rng(11)
    blocks = [np.full((8, 8), v, np.uint8) for v in range(256)]
    for _ in range(128):
        a, b = rng.integers(0, 256, 2)
        m = np.indices((8, 8)).sum(0) % 2 == 0
        blocks.append(np.where(m, a, b).astype(np.uint8))
        st = np.zeros((8, 8), np.uint8)
        st[:, :4], st[:, 4:] = a, b
        blocks.append(st)
        blocks.append(st.T.copy())
    return np.concatenate(blocks, axis=1)


@pytest.mark.parametrize("variant", [4, 3, 1])
def test_forced_kernels_adversarial_and_counter(T, dm, variant):
    """The product runs v3 (in-place ties); v2 (tie queue, stash, drains) and v1
    stay A/B kernels of the diagnostic library: each kernel forced at small sizes through the diagnostic
    library -- every quality on tie-prone blocks, random planes of
    every kind, and the fallback counter equal across kernels."""
    import oracle as O
    px = _adversarial_row()
    g = gpu_px(T, px)
    for q in range(1, 101, 3 if variant == 1 else 1):
        for ad in (0, 1):
            got = dm.Plan(q, ad, variant=variant).forward_quant(g).cpu().numpy()
            assert np.array_equal(got, O.forward_plane(px, q, ad)), (variant, q, ad)
    for trial in range(8):
        kind = ["uniform", "smooth", "const", "extreme"][trial % 4]
        q, ad = [10, 50, 75, 90, 97, 100, 1, 33][trial], trial % 2
        p = O.synth_plane(700 + trial, O.KINDS[kind], 8 * (17 + 13 * trial), 8 * (5 + 3 * trial))
        got = dm.Plan(q, ad, variant=variant).forward_quant(gpu_px(T, p)).cpu().numpy()
        assert np.array_equal(got, O.forward_plane(p, q, ad)), (variant, kind, q, ad)
    if variant == 1:  # v1 has no constant-block DC table: its exact-path count differs by design
        return
    rng = np.random.default_rng(77)
    sp = gpu_px(T, _step_blocks(rng, 48, 96))
    counts = []
    for v in (2, variant):
        plan = dm.Plan(50, 0, variant=v)
        cnt = T.zeros(1, dtype=T.int64, device="cuda")
        plan.set_fallback_counter(cnt)
        plan.forward_quant(sp)
        T.cuda.synchronize()
        counts.append(int(cnt.item()))
        plan.set_fallback_counter(None)
    assert counts[0] == counts[1] and counts[0] > 100, counts


def test_mid_size_tie_heavy_stream(T, dm):
    """More than 4096 64-block batches of tie-heavy content: step blocks (a quarter
    of the DCs are exact ties), 0/255 extremes and a plane whose batches alternate
    between step blocks and uniform noise, several qualities, both modes.  Through
    the product dispatch (v3, in-place grouped passes, every plan since round 4) and
    with the v2 queue kernel forced (variant 4: both of its tie
    paths, the stage and the queue, in one launch)."""
    import oracle as O
    rng = np.random.default_rng(31)
    step = _step_blocks(rng, 270, 1024)  # 276 480 blocks = 4320 batches
    ext = O.synth_plane(5, O.KINDS["extreme"], 8 * 1024, 8 * 270)
    # batches alternating between tie-heavy (step blocks: resolved in the stage before
    # the stores) and tie-sparse (uniform noise: the queue, stash and patches) in one launch
    uni = O.synth_plane(6, O.KINDS["uniform"], 8 * 1024, 8 * 270)
    heavy = (np.arange(8 * 1024) // 512) % 2 == 0
    mixed = np.ascontiguousarray(np.where(heavy[None, :], step, uni))
    for px in (step, ext, mixed):
        g = gpu_px(T, px)
        for q, ad in [(50, 0), (10, 1), (90, 0), (100, 1)]:
            want = O.forward_plane(px, q, ad, 16)
            counts = []
            for variant in (None, 4):
                plan = dm.Plan(q, ad, variant=variant)
                cnt = T.zeros(1, dtype=T.int64, device="cuda")
                plan.set_fallback_counter(cnt)
                got = plan.forward_quant(g).cpu().numpy()
                plan.set_fallback_counter(None)
                assert np.array_equal(got, want), (q, ad, variant)
                counts.append(int(cnt.item()))
            assert counts[0] == counts[1], (q, ad, counts)  # every flagged coefficient, either kernel
            if q == 50 and px is step:
                assert counts[0] > 1000


def test_plans_cheap_and_stash_per_stream(T, dm):
    """VERDICT r02 item 6 / ADVICE r02: a plan holds only its tables; the forward's
    tie stash is one per (device, stream), allocated lazily and sized to the
    launched grid.  100 plans (q 1..100) cost < 1 GiB of device memory; a
    multi-batch-per-wave forward of every tenth of them on ONE stream adds one
    stash (<= 256 MiB); the same plan on two streams at once (each stream its
    own stash) gives the oracle's coefficients on both."""
    import oracle as O
    # 388 800 blocks: > 16 waves x 256 CUs of batches (until round 4 tie-heavy plans ran the v2 queue kernel
    # with its stash here; every plan runs v3 now, so the product adds no stash at all)
    px = dm.synth(4242, "uniform", 3840, 2160, 3)
    outs = [T.empty((3 * 480 * 270, 64), dtype=T.int16, device="cuda") for _ in range(2)]
    T.cuda.synchronize()
    free0 = T.cuda.mem_get_info()[0]
    plans = [dm.Plan(q, q % 2) for q in range(1, 101)]
    T.cuda.synchronize()
    free1 = T.cuda.mem_get_info()[0]
    assert free0 - free1 < (1 << 30), (free0 - free1) / 2 ** 20
    side = T.cuda.Stream()
    for p in plans[::10] + plans[96:]:  # v3 (no stash), q97..q100 included
        p.forward_quant(px, out=outs[0])
    T.cuda.synchronize()
    free2 = T.cuda.mem_get_info()[0]
    # the product forward (v3 for every plan) allocates nothing: allocator slack only
    assert free1 - free2 <= (16 << 20), (free1 - free2) / 2 ** 20
    nb = 3 * 480 * 270 // 64
    for q in list(range(1, 101, 10)) + [97, 98, 99, 100]:
        for ad in (0, 1):
            assert dm.forward_kernel(q, ad, nb, 256).startswith("fdct8_quant_v3"), (q, ad)
    p = plans[98]  # q99, adaptive
    side.wait_stream(T.cuda.current_stream())
    p.forward_quant(px, out=outs[0])
    with T.cuda.stream(side):
        p.forward_quant(px, out=outs[1], stream=side)
    T.cuda.synchronize()
    host = px.cpu().numpy()
    want = np.concatenate([O.forward_plane(host[f], 99, 1, 8) for f in range(3)])
    assert np.array_equal(outs[0].cpu().numpy(), want)
    assert np.array_equal(outs[1].cpu().numpy(), want)


def test_batched_calls_do_not_serialise_and_leave_rand_alone(T, dm):
    """the batched entry points keep no process-wide lock and do
    not swap glibc's random state after a thread's first call of an entry point on a
    stream (the reference API is reentrant, src/quantization.c:8 is its
    only static, and const).  Thread A waits inside dctq_synchronize for a queue of
    forwards on its stream while thread B completes forward launches on another
    stream INSIDE that wait (the round-4 library serialised them behind A), and a
    third thread calling rand() throughout draws exactly glibc's seed-1 sequence."""
    import threading
    import time
    libc = C.CDLL("libc.so.6")
    libc.rand.restype = C.c_int
    libc.srand(1)
    want = [libc.rand() for _ in range(200000)]
    L = dm.lib()
    plan = dm.Plan(50, 0)
    big = dm.synth(777, "uniform", 3840, 2160, 64)
    small = dm.synth(778, "uniform", 64, 64, 1)
    out_big = T.empty((64 * 480 * 270, 64), dtype=T.int16, device="cuda")
    out_small = T.empty((64, 64), dtype=T.int16, device="cuda")
    sa, sb = T.cuda.Stream(), T.cuda.Stream()
    T.cuda.synchronize()
    ready, go = threading.Barrier(3), threading.Event()
    res, errs = {}, []

    def thread_a():
        try:
            plan.forward_quant(big, out=out_big, stream=sa)  # first calls of this thread on sa: isolated
            dm._check(L.dctq_synchronize(C.c_void_p(sa.cuda_stream)), L)
            ready.wait()
            go.wait()
            for _ in range(30):  # ~10 ms of GPU work queued on sa
                plan.forward_quant(big, out=out_big, stream=sa)
            t0 = time.perf_counter()
            dm._check(L.dctq_synchronize(C.c_void_p(sa.cuda_stream)), L)
            res["a"] = (t0, time.perf_counter())
        except BaseException as e:  # noqa: BLE001
            errs.append(repr(e))

    def thread_b():
        try:
            plan.forward_quant(small, out=out_small, stream=sb)
            dm._check(L.dctq_synchronize(C.c_void_p(sb.cuda_stream)), L)
            ready.wait()
            go.wait()
            done = []
            t_end = time.perf_counter() + 0.5
            while time.perf_counter() < t_end and "a" not in res:
                plan.forward_quant(small, out=out_small, stream=sb)
                done.append(time.perf_counter())
            res["b"] = done
        except BaseException as e:  # noqa: BLE001
            errs.append(repr(e))

    def thread_r():
        ready.wait()
        libc.srand(1)
        got = []
        go.set()
        while ("a" not in res or "b" not in res) and len(got) < len(want) and not errs:
            got.append(libc.rand())
        res["r"] = got

    import sys
    sw = sys.getswitchinterval()
    sys.setswitchinterval(1e-4)  # hand the GIL around often: B's launch loop is Python
    try:
        th = [threading.Thread(target=f) for f in (thread_a, thread_b, thread_r)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
    finally:
        sys.setswitchinterval(sw)
    assert not errs, errs
    t0, t1 = res["a"]
    inside = [t for t in res["b"] if t0 < t < t1]
    assert t1 - t0 > 2e-3, (t1 - t0)
    assert len(inside) >= 20, (len(inside), len(res["b"]), (t1 - t0) * 1e3)
    got = res["r"]
    assert len(got) > 1000 and got == want[:len(got)], len(got)
    T.cuda.synchronize()


class _RawStream:
    """A raw hipStream_t handle as a stream argument (Plan methods read .cuda_stream)."""

    def __init__(self, handle):
        self.cuda_stream = handle


def _hip():
    """The HIP runtime this process loaded (PyTorch's libamdhip64.so.7, shared with libdct_amd.so)."""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamCreate.restype = C.c_int
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.restype = C.c_int
    return hip


class _HostRandShield:
    """The test's OWN HIP calls (stream create / destroy) with glibc's random state
    swapped out, so that only the library's calls can disturb the host's sequence."""

    def __init__(self, libc):
        self.libc = libc
        self.libc.setstate.restype = C.c_void_p
        self.libc.setstate.argtypes = [C.c_void_p]
        self.libc.initstate.restype = C.c_void_p
        self.libc.initstate.argtypes = [C.c_uint, C.c_void_p, C.c_size_t]
        self.buf = C.create_string_buffer(256)
        self.first = True

    def __enter__(self):
        if self.first:
            self.saved = self.libc.initstate(7, self.buf, 256)
            self.first = False
        else:
            self.saved = self.libc.setstate(self.buf)

    def __exit__(self, *exc):
        self.libc.setstate(self.saved)
        return False


def test_many_streams_rand_and_results(T, dm):
    """a host that keeps creating streams.  150 DISTINCT raw streams
    (hipStreamCreate; torch.cuda.Stream() recycles a pool of 32), all alive at once:
    past 64 (device, stream) pairs a thread's launch-isolation list is cleared and
    each stream's next first call is isolated again -- every result stays bit-exact,
    and glibc's seed-1 sequence drawn between the launches is undisturbed."""
    libc = C.CDLL("libc.so.6")
    libc.rand.restype = C.c_int
    libc.srand(1)
    want = [libc.rand() for _ in range(600)]
    hip = _hip()
    shield = _HostRandShield(libc)
    L = dm.lib()
    plan = dm.Plan(50, 0)
    px = dm.synth(4040, "uniform", 256, 128, 1)
    ref = plan.forward_quant(px)
    T.cuda.synchronize()
    outs = [T.empty_like(ref) for _ in range(150)]
    handles = []
    with shield:
        for _ in range(150):
            h = C.c_void_p()
            assert hip.hipStreamCreate(C.byref(h)) == 0
            handles.append(h.value)
    assert len(set(handles)) == 150
    T.cuda.synchronize()
    libc.srand(1)
    got = []
    for rep in range(2):  # the second pass runs after the list was cleared by the first
        for h, o in zip(handles, outs):
            plan.forward_quant(px, out=o, stream=_RawStream(h))
            got.append(libc.rand())
    for h in handles:
        dm._check(L.dctq_synchronize(C.c_void_p(h)), L)
    assert got == want[:len(got)]
    assert all(T.equal(o, ref) for o in outs)
    for h in handles:  # the host protocol before hipStreamDestroy (include/dct_amd.h)
        dm._check(L.dctq_stream_release(C.c_void_p(h)), L)
    with shield:
        for h in handles:
            assert hip.hipStreamDestroy(C.c_void_p(h)) == 0


def test_stream_handle_reuse_is_isolated(T, dm):
    """streams destroyed and re-created in a loop.  The runtime
    hands out a destroyed stream's handle again; a re-created stream's first call
    must still be isolated (LaunchIsolation keys on the handle AND the runtime's
    stream id where the runtime has hipStreamGetId, and dctq_stream_release drops
    the calling thread's entry).  Both host styles -- calling dctq_stream_release
    before hipStreamDestroy, and not -- keep glibc's seed-1 sequence intact with
    bit-exact results on every stream."""
    libc = C.CDLL("libc.so.6")
    libc.rand.restype = C.c_int
    libc.srand(1)
    want = [libc.rand() for _ in range(2000)]
    hip = _hip()
    has_id = hasattr(hip, "hipStreamGetId")
    shield = _HostRandShield(libc)
    L = dm.lib()
    plan = dm.Plan(90, 1)
    px = dm.synth(4141, "smooth", 128, 64, 1)
    ref = plan.forward_quant(px)
    T.cuda.synchronize()
    out = T.empty_like(ref)
    # torch's first fill and compare kernels load their code objects, and that reaches rand():
    # both run once here, before the seed (tools/rand_probe.py: the library's own calls draw nothing)
    out.zero_()
    assert T.equal(ref, ref.clone())
    T.cuda.synchronize()
    libc.srand(1)
    got, seen, reused = [], set(), 0
    styles = ("release",) + (("no-release",) if has_id else ())
    for style in styles:
        for i in range(60):
            with shield:
                h = C.c_void_p()
                assert hip.hipStreamCreate(C.byref(h)) == 0
            reused += h.value in seen
            seen.add(h.value)
            out.zero_()
            T.cuda.synchronize()
            plan.forward_quant(px, out=out, stream=_RawStream(h.value))
            got.append(libc.rand())
            plan.forward_quant(px, out=out, stream=_RawStream(h.value))  # the steady-state call
            got.append(libc.rand())
            dm._check(L.dctq_synchronize(C.c_void_p(h.value)), L)
            assert T.equal(out, ref), (style, i)
            if style == "release":
                dm._check(L.dctq_stream_release(C.c_void_p(h.value)), L)
            with shield:
                assert hip.hipStreamDestroy(h) == 0
    assert reused > 0, "the runtime never reused a stream handle: nothing was exercised"
    assert got == want[:len(got)]


class _PerThreadStream:
    """hipStreamPerThread as a stream argument: one handle value (2), a different real stream per thread."""
    cuda_stream = 2


def test_stash_per_thread_stream_two_threads(T, dm):
    """hipStreamPerThread is one handle value but a different real
    stream on each thread.  Two threads run a tie-heavy plan (q99, the v2 queue
    kernel with its pixel stash, 4 batches per wave) concurrently on it: each
    thread's launches get their own stash, so both outputs equal the oracle;
    dctq_stream_release from each thread frees that thread's stash only."""
    import threading
    import oracle as O
    px = dm.synth(5151, "uniform", 3840, 2160, 2)
    host = px.cpu().numpy()
    want = np.concatenate([O.forward_plane(host[f], 99, 0, 8) for f in range(2)])
    plan = dm.Plan(99, 0, variant=4, num_cus=8)  # v2 forced; 1 024 waves for 4 050 batches
    outs = [T.zeros((2 * 480 * 270, 64), dtype=T.int16, device="cuda") for _ in range(2)]
    T.cuda.synchronize()
    L = dm.diag()
    errs, sizes = [], [0, 0]
    start = threading.Barrier(2)

    def work(k):
        try:
            start.wait()
            for _ in range(4):
                plan.forward_quant(px, out=outs[k], stream=_PerThreadStream())
            dm._check(L.dctq_synchronize(C.c_void_p(2)), L)
            sizes[k] = L.dctq_diag_stream_stash_bytes(C.c_void_p(2))
            dm.stream_release(_PerThreadStream(), diagnostic=True)
            assert L.dctq_diag_stream_stash_bytes(C.c_void_p(2)) == 0
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert sizes[0] > 0 and sizes[1] > 0, sizes  # each thread had its own stash
    for k in range(2):
        got = outs[k].cpu().numpy()
        assert np.array_equal(got, want), (k, int((got != want).sum()))


def test_stash_captured_launch_survives_grow(T, dm):
    """a forward captured into a graph keeps a stash of its own.  A
    small tie-heavy launch (q99, v2) is captured, then a LARGER direct launch on the
    same stream grows (frees and reallocates) the stream's stash, then the graph
    is replayed: its output still equals the oracle.  Released at the end."""
    import oracle as O
    small = dm.synth(6161, "uniform", 1920, 1080, 2)
    big = dm.synth(6262, "uniform", 3840, 2160, 2)
    plan_small = dm.Plan(99, 1, variant=4, num_cus=2)  # a small grid: a small stash
    plan_big = dm.Plan(99, 1, variant=4, num_cus=64)  # a larger grid: grows the stream's stash
    out_s = T.zeros((2 * 240 * 135, 64), dtype=T.int16, device="cuda")
    out_b = T.zeros((2 * 480 * 270, 64), dtype=T.int16, device="cuda")
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(s):
        plan_small.forward_quant(small, out=out_s, stream=s)  # a live stash sized for the small grid
    s.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g, stream=s):
        plan_small.forward_quant(small, out=out_s, stream=s)
    L = dm.diag()
    before = L.dctq_diag_stream_stash_bytes(C.c_void_p(s.cuda_stream))
    with T.cuda.stream(s):
        plan_big.forward_quant(big, out=out_b, stream=s)
    s.synchronize()
    assert L.dctq_diag_stream_stash_bytes(C.c_void_p(s.cuda_stream)) > before > 0
    out_s.zero_()
    T.cuda.synchronize()
    g.replay()
    g.replay()
    T.cuda.synchronize()
    hs, hb = small.cpu().numpy(), big.cpu().numpy()
    assert np.array_equal(out_s.cpu().numpy(), np.concatenate([O.forward_plane(hs[f], 99, 1, 8) for f in range(2)]))
    assert np.array_equal(out_b.cpu().numpy(), np.concatenate([O.forward_plane(hb[f], 99, 1, 8) for f in range(2)]))
    del g
    dm.stream_release(s, diagnostic=True)
    assert L.dctq_diag_stream_stash_bytes(C.c_void_p(s.cuda_stream)) == 0


def _tail(err: str) -> str:
    """A failed bench's stderr: its progress lines (DCTQ_BENCH_TRACE) and the end."""
    marks = [ln for ln in err.splitlines() if ln.startswith("[bench rank") or "Error" in ln or "error:" in ln]
    return "\n".join(marks[-40:]) + "\n...\n" + err[-2000:]


def test_bench_gpus2_gloo(T, dm):
    """bench.py --gpus 2 with no launcher forms a 2-rank world by itself (its
    children share this box's one GPU over gloo, as a rehearsal of the driver's
    8-GPU run): the line says n_gpus 2 / world_size 2, the gather leg's own
    slice survives the exchange, and the band split of one 4K 4:2:0 frame
    gathers to the unsharded forward."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env["DCTQ_BENCH_TRACE"] = "1"
    cmd = [sys.executable, "bench.py", "--full", "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1",
           "--no-cpu", "--frames", "2", "--total-frames", "4", "--gather-steps", "2", "--round-trip-steps", "1",
           "--encode-steps", "1", "--ceiling-rounds", "0", "--prewarm-ms", "0"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, _tail(r.stderr)
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]  # stdout: the one JSON line only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["backend"] == "gloo", d["config"]
    g, b = d["gather"], d["band"]
    assert g["world_size"] == 2 and g["own_slice_intact"] is True, g
    assert b["gathered_equals_unsharded"] is True, b
    assert g["xgmi"]["bytes_received_per_rank"] == g["bytes_received_per_rank"] > 0, g
    assert b["xgmi"]["achieved_GBs_per_rank"] > 0, b
    # the direct-push shape at world 2: the same coefficients as the all-gather, band equal to unsharded
    assert g["methods_gather_the_same"] is True and g["methods"]["p2p"]["own_slice_intact"] is True, g
    assert b["methods"]["p2p"]["gathered_equals_unsharded"] is True, b
    assert g["methods"]["p2p"]["xgmi"]["bytes_received_per_rank"] == g["bytes_received_per_rank"], g
    # the gather leg checks each shape's result against the unsharded forward, every rank
    assert g["gathered_equals_unsharded"] is True and g["fault_injected"] == "none", g
    for m in ("all_gather", "p2p"):
        assert g["methods"][m]["gathered_equals_unsharded"] is True, (m, g)
    # ... and a wrong shard offset shared by both shapes fails it (both shapes still agree)
    cmd_f = cmd + ["--gather-fault", "offset", "--round-trip-steps", "0", "--encode-steps", "0"]
    r = subprocess.run(cmd_f, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, _tail(r.stderr)
    g = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])["gather"]
    assert g["fault_injected"] == "offset" and g["methods_gather_the_same"] is True, g
    assert g["gathered_equals_unsharded"] is False, g
    assert not any(g["methods"][m]["gathered_equals_unsharded"] for m in ("all_gather", "p2p")), g
    # a p2p peer that stalls past the process-group timeout and then fails.
    # The p2p legs run last and fail soft: the line still carries the headline, the all-gather
    # legs' results and the p2p leg's error, within a bounded time, and every rank exits 0.
    import time
    cmd_s = cmd + ["--gather-fault", "p2p-stall", "--dist-timeout", "15", "--round-trip-steps", "0",
                   "--encode-steps", "1"]
    t0 = time.time()
    r = subprocess.run(cmd_s, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, _tail(r.stderr)
    assert time.time() - t0 < 200
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["roofline"]["frac"] > 0 and d["n_gpus"] == 2, d
    lg = d["legs"]
    assert lg["gather.all_gather"]["ok"] and lg["band.all_gather"]["ok"] and lg["encode.symbol_gather"]["ok"], lg
    assert "error" in lg["gather.p2p"] and "skipped" in lg["band.p2p"], lg
    g, b = d["gather"], d["band"]
    assert g["methods"]["all_gather"]["gathered_equals_unsharded"] is True and "error" in g["methods"]["p2p"], g
    assert b["methods"]["all_gather"]["gathered_equals_unsharded"] is True and "skipped" in b["methods"]["p2p"], b
    assert d["encode"]["gather_blocks_per_s"] > 0, d["encode"]


def test_dist_legs_rccl_one_rank(T, dm):
    """The N>1 legs of bench.py over a real RCCL process group: one rank on this GPU
    (bench.py --dist-legs).  The gather leg (BASELINE configs[3]: all_gather_into_tensor
    of the coefficient planes), the band split of one 4K 4:2:0 frame (its three planes
    in one gather, checked against an unsharded forward) and the encoder's symbol-stream gather run
    end to end through the nccl backend, in a child process with a time limit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "bench.py", "--full", "--dist-legs", "--steps", "2", "--warmup", "1", "--no-cpu", "--frames", "2",
           "--total-frames", "2", "--gather-steps", "2", "--round-trip-steps", "0", "--encode-steps", "1",
           "--ceiling-rounds", "0", "--prewarm-ms", "0"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _tail(r.stderr)
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["config"]["world_size"] == 1 and d["n_gpus"] == 1
    g, b, e = d["gather"], d["band"], d["encode"]
    assert "RCCL" in g["op"] and g["own_slice_intact"] and g["world_size"] == 1, g
    assert "RCCL" in b["op"] and b["gathered_equals_unsharded"], b
    # both of SURVEY 8(e)'s shapes ran through RCCL: the all-gather and the grouped send/recv pushes
    for leg in (g, b):
        assert set(leg["methods"]) == {"all_gather", "p2p"}, leg
        assert "ncclSend/ncclRecv" in leg["methods"]["p2p"]["op"], leg
        assert leg["methods"]["p2p"]["xgmi"]["us_per_gather"] > 0, leg
    assert g["methods_gather_the_same"] and g["methods"]["p2p"]["own_slice_intact"], g
    assert b["methods"]["p2p"]["gathered_equals_unsharded"], b
    assert "RCCL" in e["gather_op"] and e["gather_blocks_per_s"] > 0, e


def test_bench_json_contract(T, dm):
    """bench.py's one JSON line carries what the round driver reads (the metric, the
    whole-job value, the timing fields, config.workload, the roofline object with
    bound/achieved/peak/unit/frac/traffic, the CPU baseline with value/unit/cores/
    kind/sample) and its own parity check passes; a short run in a child process."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--frames", "2", "--cpu-seconds", "2",
           "--ceiling-rounds", "1", "--round-trip-steps", "1", "--encode-steps", "1", "--prewarm-ms", "20"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _tail(r.stderr)
    lines = [x for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["blocks_per_gpu_step"]) < 1e-3 * d["value"]
    assert "workload" in d["config"]
    ro = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in ro, k
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and 0 < ro["frac"] < 1
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-9
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "reference" and cb["value"] > 0 and cb["cores"] >= 1
    assert d["parity_check"] is True and d["encode"]["huffman"]["parity_check_chroma0"] is True
    rt = d["round_trip"]
    assert rt["parity_check"] is True, rt.get("parity")
    mc = rt["movement_ceiling"]
    assert 0 < mc["fused_frac"] < 1 and 0 < mc["movement_frac"] < 1 and 0 < mc["flat_124_frac"] < 1, mc


def test_bench_plain_run_and_dump_outputs(T, dm, tmp_path):
    """bench.py without --full measures the headline only (every other leg's key is null,
    no leg ran), --steps is the number of timed steps that ms_per_step averages over, and
    --dump-outputs writes the last timed step's coefficient planes: float32 .npy files that
    equal a forward of the same seeded frames in this process, block for block (one frame:
    under the size budget, so every block is written)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, _tail(r.stderr)
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "macroblocks/s" and d["dtype"] == "fp32" and d["metric"].startswith("8x8 macroblocks/sec")
    nblk = d["config"]["blocks_per_gpu_step"]
    assert nblk == 194400 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - nblk) < 1e-3 * d["value"]
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["movement_ceiling"] is None
    for k in ("cpu_baseline", "parity_check", "gather", "band", "round_trip", "encode", "small_frame",
              "legacy_per_block", "gpu"):
        assert d[k] is None, k
    assert d["legs"] == {}
    assert sorted(os.listdir(tmp_path)) == ["chroma_coef.npy", "luma_coef.npy"]
    luma = dm.synth(12345, "uniform", 3840, 2160, 1)
    chroma = dm.synth(12345 + 50000, "uniform", 1920, 1080, 2)
    want = dm.Plan(50, 0).forward_quant_planes([luma, chroma])
    for name, w in zip(("luma_coef", "chroma_coef"), want):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(w.shape), (name, got.dtype, got.shape)
        assert d["dump_outputs"]["files"][name + ".npy"]["blocks"] == w.shape[0]
        assert np.array_equal(got, w.cpu().numpy().astype(np.float32)), name


def test_diag_stream_moves_bytes(T, dm):
    """The hardware-ceiling streams of the diagnostic library (bench.py
    roofline.movement_ceiling) move what they claim: the flat 1:2 stream writes
    each 1 KiB input chunk twice (the second copy with bit 0 of its first dword
    flipped), the write-only stream covers the whole output; the round trip's 1:2:4
    streams (kinds 5, 8-13, 15-17) and the plane-read 1:2 stream (14) run and write."""
    D = dm.diag()
    n = 64 * 40
    src = T.randint(0, 256, (n * 64,), dtype=T.uint8, device="cuda")
    s = T.cuda.current_stream().cuda_stream
    for kind in (0, 1):
        dst = T.zeros(n * 128, dtype=T.uint8, device="cuda")
        assert D.dctq_diag_stream(kind, src.data_ptr(), dst.data_ptr(), n, s) == 0
        T.cuda.synchronize()
        a = src.view(-1, 4, 1024).cpu().numpy()
        b = dst.view(-1, 8, 1024).cpu().numpy()
        assert np.array_equal(b[:, :4], a)
        flip = b[:, 4:].copy().view(np.uint32)
        flip.reshape(-1, 4)[:, 0] ^= 1
        assert np.array_equal(flip.view(np.uint8).reshape(a.shape), a)
    for kind in (3, 4):
        dst = T.zeros(n * 128, dtype=T.uint8, device="cuda")
        assert D.dctq_diag_stream(kind, src.data_ptr(), dst.data_ptr(), n, s) == 0
        assert D.dctq_diag_stream(2, src.data_ptr(), dst.data_ptr(), n, s) == 0
        T.cuda.synchronize()
        w = dst.view(-1, 16).cpu().numpy().view(np.uint32)
        assert (w[:, 2] == 7).all() and (w[:, 3] == 9).all()
    # the round trip's streams (1:2:4 bytes): the same bytes in the two-array layout with
    # and without the drained store groups; the plane-read streams in any batch order
    out = {}
    for kind in (5, 8, 9, 10, 11, 12, 13, 15, 16, 17):
        dst = T.zeros(n * 384, dtype=T.uint8, device="cuda")
        assert D.dctq_diag_stream(kind, src.data_ptr(), dst.data_ptr(), n, s) == 0, kind
        T.cuda.synchronize()
        out[kind] = dst.cpu().numpy()
        assert out[kind].any(), kind
    assert np.array_equal(out[8], out[9]) and np.array_equal(out[9], out[16])
    assert np.array_equal(out[11], out[12]) and np.array_equal(out[11], out[13]) and np.array_equal(out[11], out[17])
    a = src.view(-1, 4, 1024).cpu().numpy()  # kind 8: region A holds each batch's 4 KiB twice (bit 0 of dword 0 flipped)
    ra = out[8][:n * 128].reshape(-1, 8, 1024)
    assert np.array_equal(ra[:, 0::2], a)
    dst = T.zeros(n * 128, dtype=T.uint8, device="cuda")
    assert D.dctq_diag_stream(14, src.data_ptr(), dst.data_ptr(), n, s) == 0
    T.cuda.synchronize()
    assert dst.cpu().numpy().any()
    assert D.dctq_diag_stream(18, src.data_ptr(), dst.data_ptr(), n, s) != 0


def _sym32(sym):
    """An encoder symbol tensor (int32: 4-byte format, int16: 2-byte format) as 4-byte symbols."""
    import oracle as O
    a = sym.cpu().numpy()
    return O.unpack16(a.view(np.uint16)) if a.dtype == np.int16 else a.view(np.uint32)


def _step_blocks(rng, by, bx):
    """Left/right two-level blocks: a quarter of their DCs are exact rounding ties at q50."""
    ab = rng.integers(0, 256, (by, bx, 2), dtype=np.uint8)
    blk = np.concatenate([np.repeat(ab[:, :, :1, None], 4, 3).repeat(8, 2),
                          np.repeat(ab[:, :, 1:, None], 4, 3).repeat(8, 2)], axis=3)
    return np.ascontiguousarray(blk.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8))


def _tie_count_plane(rng, counts):
    """One 64-block batch per block row: row r holds counts[r] two-level step blocks whose
    DC is an exact rounding tie at q50 (a != b, a + b = 2 mod 4: one exact-path entry
    each), the rest constant blocks (their DC ties go to the constant-block table, not
    the exact path).  So batch r's tie pass has exactly counts[r] entries."""
    px = np.empty((8 * len(counts), 8 * 64), np.uint8)
    for r, n in enumerate(counts):
        vals = rng.integers(0, 256, 64)
        pos = set(rng.choice(64, n, replace=False).tolist())
        for b in range(64):
            blk = np.full((8, 8), vals[b], np.uint8)
            if b in pos:
                while True:
                    a, c = rng.integers(0, 256, 2)
                    if a != c and (int(a) + int(c)) % 4 == 2:
                        break
                blk[:, :4], blk[:, 4:] = a, c
            px[8 * r:8 * r + 8, 8 * b:8 * b + 8] = blk
    return px


def test_grouped_tie_passes(T, dm):
    """Tie passes of 0..64 entries per batch around every grouped path's bound (<= 8
    entries: 8 lanes per entry; 9..16 and 17..32 in the kernels with wide rounds, the
    fused Huffman sizes: 4 and 2 lanes per entry, the forward without counter or variance
    output: 2 lanes per entry for 9..32; above: one entry per lane;
    exact_grouped<G>) in every kernel that resolves ties in place -- the forward (v3;
    v2 forced beside it), the fused round trip, the encoder and the fused Huffman
    sizes -- for both modes, with the fallback counter counting every entry once."""
    import oracle as O
    rng = np.random.default_rng(77)
    counts = [0, 1, 2, 3, 5, 7, 8, 9, 12, 15, 16, 17, 20, 24, 31, 32, 33, 40, 48, 63, 64, 8, 1, 16] * 2
    px = _tie_count_plane(rng, counts)
    g = gpu_px(T, px)
    for ad in (0, 1):
        want = O.forward_plane(px, 50, ad)
        got = {}
        for variant in (None, 4):
            plan = dm.Plan(50, ad, variant=variant)
            cnt = T.zeros(1, dtype=T.int64, device="cuda")
            plan.set_fallback_counter(cnt)
            got[variant] = plan.forward_quant(g).cpu().numpy()
            plan.set_fallback_counter(None)
            assert np.array_equal(got[variant], want), (ad, variant)
            assert int(cnt.item()) >= sum(counts), (ad, variant, int(cnt.item()))
        plan = dm.Plan(50, ad)
        # without the counter: the product's v3 instantiation, whose passes of 9..32 entries run 2 lanes
        # per entry (the counted one keeps one entry per lane: it spills with the wide rounds)
        assert np.array_equal(plan.forward_quant(g).cpu().numpy(), want), ad
        coefs, recons = plan.round_trip_planes([g])
        assert np.array_equal(T.cat(coefs).cpu().numpy(), want), ad
        ec, off, sym = plan.encode_planes([g])
        assert np.array_equal(T.cat(ec).cpu().numpy(), want), ad
        woff, wsym = O.rle_encode_plane(want)
        assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), ad
        assert np.array_equal(_sym32(sym), wsym), ad
        bits = plan.huffman_bits_planes([g]).cpu().numpy().view(np.uint32)
        assert np.array_equal(bits, O.huffman_bits_plane(want)), ad


def test_forward_quant_planes(T, dm):
    """One launch over up to 4 planes of different geometry (ragged block counts, a
    multi-frame stack, a single block) equals per-plane calls and the oracle,
    including var_num and tie-heavy planes whose exact-path entries share a queue."""
    import oracle as O
    rng = np.random.default_rng(21)
    sets = [
        [O.synth_plane(1, 0, 8 * 65, 8 * 9), _step_blocks(rng, 7, 13),
         O.synth_plane(2, 3, 8, 8), _step_blocks(rng, 33, 61)],
        [_step_blocks(rng, 40, 40), O.synth_plane(3, 1, 8 * 20, 8 * 12)],
        [O.synth_plane(4, 0, 8 * 129, 8 * 3)],
    ]
    for q, ad in [(50, 0), (50, 1), (90, 0), (7, 1)]:
        plan = dm.Plan(q, ad)
        for planes in sets:
            gp = [gpu_px(T, p) for p in planes]
            vns = [T.zeros(p.size // 64, dtype=T.int32, device="cuda") for p in planes]
            outs = plan.forward_quant_planes(gp, var_nums=vns)
            for p, o, v in zip(planes, outs, vns):
                assert np.array_equal(o.cpu().numpy(), O.forward_plane(p, q, ad)), (q, ad, p.shape)
                assert np.array_equal(v.cpu().numpy().astype(np.float64) / 4096.0, O.plane_variance(p))
            outs2 = plan.forward_quant_planes(gp)  # no var_num
            for p, o in zip(planes, outs2):
                assert np.array_equal(o.cpu().numpy(), O.forward_plane(p, q, ad)), (q, ad, p.shape)
    # a frame stack as one of the planes
    F, H, W = 3, 24, 40
    stack = np.stack([O.synth_plane(50 + f, f % 4, W, H) for f in range(F)])
    luma = O.synth_plane(60, 0, 8 * 31, 8 * 5)
    outs = dm.Plan(75, 1).forward_quant_planes([gpu_px(T, stack), gpu_px(T, luma)])
    want = np.concatenate([O.forward_plane(stack[f], 75, 1) for f in range(F)])
    assert np.array_equal(outs[0].cpu().numpy(), want)
    assert np.array_equal(outs[1].cpu().numpy(), O.forward_plane(luma, 75, 1))
    # argument checks: 0 or 5 planes, a NULL var_num entry
    g = gpu_px(T, luma)
    plan = dm.Plan(50, 0)
    with pytest.raises(dm.DctqError):
        plan.forward_quant_planes([g] * 5)
    with pytest.raises(dm.DctqError):
        plan.forward_quant_planes([])
    L = dm.lib()
    d = (dm._Plane * 1)(dm.plane_desc(g))
    o = T.empty((luma.size // 64, 64), dtype=T.int16, device="cuda")
    cp = (C.c_void_p * 1)(o.data_ptr())
    vp = (C.c_void_p * 1)(None)
    rc = L.dctq_forward_quant_planes(plan._h, d, 1, C.cast(cp, C.c_void_p), C.cast(vp, C.c_void_p), None)
    assert rc != 0


def test_forward_float_tolerance(T, dm, tiles):
    import oracle as O
    for kind in ["uniform", "smooth", "const", "extreme"]:
        px = tiles[f"{kind}_px"]
        got = dm.Plan(50, 0).forward_float(gpu_px(T, px)).cpu().numpy().astype(np.float64)
        assert np.abs(got[:32] - tiles[f"{kind}_forward32"]).max() <= 1e-4, kind
        _, want = O.forward_plane(px, 50, 0, want_float=True)
        assert np.abs(got - want).max() <= 1e-4, kind


def test_inverse_round_trip(T, dm):
    import oracle as O
    for kind in ["uniform", "smooth"]:
        px = O.synth_plane(21, O.KINDS[kind], 256, 128)
        for q, ad in [(50, 0), (50, 1), (90, 0), (10, 1), (100, 0)]:
            plan = dm.Plan(q, ad)
            vn = T.zeros(px.size // 64, dtype=T.int32, device="cuda")
            coef = plan.forward_quant(gpu_px(T, px), var_num=vn)
            rec = plan.inverse(coef, var_num=vn).cpu().numpy().astype(np.float64)
            want = O.inverse_plane(coef.cpu().numpy(), q, ad, O.plane_variance(px) if ad else None) + 128.0
            assert np.abs(rec - want).max() <= 1e-4, (kind, q, ad, np.abs(rec - want).max())


def test_float_and_inverse_ragged_geometries(T, dm):
    """The fp64 kernels process 32 blocks per wave (two lanes per block): block
    counts that are not multiples of 32, multi-frame stacks and padded rows."""
    import oracle as O
    for (w, h, nf, pad) in [(8, 8, 1, 0), (40, 24, 1, 0), (264, 8, 1, 8), (136, 56, 3, 16), (1920, 16, 2, 0)]:
        frames = [O.synth_plane(70 + f, O.KINDS["uniform"], w, h) for f in range(nf)]
        buf = np.zeros((nf, h, w + pad), np.uint8)
        for f in range(nf):
            buf[f, :, :w] = frames[f]
        g = T.from_numpy(buf).cuda()[:, :, :w]
        for q, ad in [(50, 0), (75, 1)]:
            plan = dm.Plan(q, ad)
            ff = plan.forward_float(g).cpu().numpy().astype(np.float64)
            want_f = np.concatenate([O.forward_plane(fr, q, ad, want_float=True)[1].reshape(-1, 64) for fr in frames])
            assert np.abs(ff - want_f).max() <= 1e-4, (w, h, nf, q, ad)
            vn = T.zeros(nf * (w // 8) * (h // 8), dtype=T.int32, device="cuda")
            coef = plan.forward_quant(g, var_num=vn)
            rec = plan.inverse(coef, var_num=vn).cpu().numpy().astype(np.float64)
            c = coef.cpu().numpy()
            per = (w // 8) * (h // 8)
            want = np.concatenate([
                O.inverse_plane(c[f * per:(f + 1) * per], q, ad, O.plane_variance(frames[f]) if ad else None)
                for f in range(nf)]) + 128.0
            assert np.abs(rec - want).max() <= 1e-4, (w, h, nf, q, ad)


def test_round_trip_planes_fused(T, dm):
    """dctq_round_trip_planes (one launch, forward + inverse fused through LDS):
    coefficients bit-exact with the oracle, recon within 1e-4 of the oracle's
    dct_inverse(dequantize()), over ragged planes (block counts not multiples of
    32/64), a frame stack, tie-heavy step-block planes (exact path inside the
    fused kernel) and adaptive plans; var_num optional."""
    import oracle as O
    rng = np.random.default_rng(33)
    planes = [O.synth_plane(5, 0, 8 * 65, 8 * 9), _step_blocks(rng, 7, 13), O.synth_plane(6, 1, 8, 8),
              _step_blocks(rng, 17, 47)]
    F, H, W = 3, 24, 40
    stack = np.stack([O.synth_plane(80 + f, f % 4, W, H) for f in range(F)])
    for q, ad in [(50, 0), (50, 1), (90, 1), (10, 0), (100, 1)]:
        plan = dm.Plan(q, ad)
        for ps in (planes, [stack, planes[0]]):
            gp = [gpu_px(T, p) for p in ps]
            vns = [T.zeros(p.size // 64, dtype=T.int32, device="cuda") for p in ps]
            coefs, recs = plan.round_trip_planes(gp, var_nums=vns)
            coefs2, recs2 = plan.round_trip_planes(gp)
            for p, c, r, v, c2, r2 in zip(ps, coefs, recs, vns, coefs2, recs2):
                frames = list(p) if p.ndim == 3 else [p]
                want_c = np.concatenate([O.forward_plane(f, q, ad) for f in frames])
                want_v = np.concatenate([O.plane_variance(f) for f in frames])
                got_c = c.cpu().numpy()
                assert np.array_equal(got_c, want_c), (q, ad, p.shape)
                assert np.array_equal(c2.cpu().numpy(), want_c)
                assert np.array_equal(v.cpu().numpy().astype(np.float64) / 4096.0, want_v)
                want_r = O.inverse_plane(want_c, q, ad, want_v if ad else None) + 128.0
                err = np.abs(r.cpu().numpy().astype(np.float64) - want_r).max()
                assert err <= 1e-4, (q, ad, p.shape, err)
                assert np.array_equal(r.cpu().numpy(), r2.cpu().numpy())
                # and the unfused dctq_inverse's floats (fp64 arithmetic: half an fp32 ulp from
                # the reference), within the fused kernel's own bound when it runs the fp32 inverse
                ri = plan.inverse(c, var_num=v).cpu().numpy()
                bound, f32 = dm.inverse_bound(q, ad)
                assert np.abs(ri - r.cpu().numpy()).max() <= (bound + 2e-5 if f32 else 2e-5), (q, ad, f32)


@pytest.mark.parametrize("ad", [0, 1])
def test_round_trip_full_size_4k420(T, dm, ad):
    """BASELINE configs[4] at full size: round_trip_planes over 16 4K 4:2:0 frames
    (bench.py's seeds and multi-plane launch: 3.1 M blocks, so the x8 grid gives
    its waves more than one batch each), every block checked -- coefficients
    bit-exact against the oracle's forward_plane, recon within 1e-4 of its
    dct_inverse(dequantize()) + 128 -- and luma frame 0's PSNR equal to the
    oracle pipeline's with the reference formula (tests/test_entropy.c:368-393;
    src/quantization.c:133-151, src/dct.c:80-105)."""
    import math
    import oracle as O
    F, q = 16, 50
    luma = dm.synth(12345, "uniform", 3840, 2160, F)
    chroma = dm.synth(12345 + 50000, "uniform", 1920, 1080, 2 * F)
    (cy, cc), (ry, rc) = dm.Plan(q, ad).round_trip_planes([luma, chroma])
    assert (luma.shape[0] * 480 * 270 + chroma.shape[0] * 240 * 135) // 64 > 8 * 4 * 4 * 256  # > 1 batch per wave
    threads = min(16, os.cpu_count() or 1)
    psnr_gpu = psnr_ref = None
    for px, coef, rec, per in ((luma, cy, ry, 480 * 270), (chroma, cc, rc, 240 * 135)):
        host_px = px.cpu().numpy()
        for f in range(px.shape[0]):
            got_c = coef[f * per:(f + 1) * per].cpu().numpy()
            got_r = rec[f * per:(f + 1) * per].cpu().numpy().astype(np.float64)
            want_c = O.forward_plane(host_px[f], q, ad, threads)
            assert np.array_equal(got_c, want_c), (ad, tuple(px.shape), f, int((got_c != want_c).sum()))
            want_r = O.inverse_plane(want_c, q, ad, O.plane_variance(host_px[f]) if ad else None) + 128.0
            err = float(np.abs(got_r - want_r).max())
            assert err <= 1e-4, (ad, tuple(px.shape), f, err)
            if px is luma and f == 0:
                h, w = host_px.shape[1:]
                blocks = host_px[0].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
                blocks = blocks.astype(np.float64)

                def psnr(r):
                    mse = float(((blocks - np.clip(r, 0, 255)) ** 2).mean())
                    return 10.0 * math.log10(255.0 * 255.0 / mse)
                psnr_gpu, psnr_ref = psnr(got_r), psnr(want_r)
    assert abs(psnr_gpu - psnr_ref) <= 1e-3, (psnr_gpu, psnr_ref)
    # the bug-compatible 1/Q dequantization gives ~11 dB on noise, adaptive ~23 dB
    assert (psnr_ref < 15.0) if ad == 0 else (psnr_ref > 15.0), psnr_ref


def _basis_sign_blocks():
    """For every (u, v), the u8 block whose centred pixels are +-127/-128 with the signs
    of D[u][i] D[v][j], and its negation: each maximises |c_uv| (the bound's
    |c_uv| <= 128 L1(D_u) L1(D_v)), so its quantized coefficient and dequantized
    input to the inverse are as large as the plan allows.  A 8 x 1024 plane."""
    import oracle as O
    D = O.dct_matrix(8)
    blocks = []
    for u in range(8):
        for v in range(8):
            sg = np.where(np.outer(D[u], D[v]) >= 0, 1, -1)
            blocks += [128 + 127 * sg, 128 - 128 * sg]
    b = np.clip(np.array(blocks), 0, 255).astype(np.uint8)  # [128, 8, 8]
    return np.ascontiguousarray(b.transpose(1, 0, 2).reshape(8, 128 * 8))


def test_round_trip_inverse_fp32_within_bound(T, dm):
    """The fused round trip's fp32 inverse (roundtrip8_f32): a non-adaptive plan runs
    it only when the rigorous bound of tools/inv_bound.py (plan_tables.hip
    inverse_f32_bound) keeps |recon - reference| <= 5e-5 for every input block
    (q <= 71 of the standard table).  On blocks that maximise each coefficient, noise,
    extremes, flat and smooth planes: coefficients bit-exact in both inverses, the
    fp32 inverse within its plan's bound (<= 1e-4, north_star), the forced fp64
    inverse within half an fp32 ulp of the reference (src/dct.c:80-105,
    src/quantization.c:133-151), and plans past the bound run the fp64 inverse."""
    import oracle as O
    planes = [_basis_sign_blocks(), O.synth_plane(3, O.KINDS["extreme"], 256, 64),
              O.synth_plane(4, O.KINDS["uniform"], 256, 64), O.synth_plane(5, O.KINDS["const"], 128, 64),
              O.synth_plane(6, O.KINDS["smooth"], 128, 64)]
    for q in (1, 10, 50, 71, 72, 90):
        bound, admitted = dm.inverse_bound(q, 0)
        assert admitted == (q <= 71) and admitted == (bound <= 5e-5), (q, bound)
        assert dm.inverse_bound(q, 1)[1] is False  # adaptive plans keep the fp64 inverse
        p_auto, p64 = dm.Plan(q, 0), dm.Plan(q, 0, inverse="fp64")
        for px in planes:
            g = gpu_px(T, px)
            (c,), (r,) = p_auto.round_trip_planes([g])
            (c2,), (r2,) = p64.round_trip_planes([g])
            want_c = O.forward_plane(px, q, 0)
            assert np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(c2.cpu().numpy(), want_c), q
            want_r = O.inverse_plane(want_c, q, 0) + 128.0
            got, got64 = r.cpu().numpy(), r2.cpu().numpy()
            half_ulp = np.spacing(np.abs(want_r).astype(np.float32)).astype(np.float64) / 2
            assert (np.abs(got64.astype(np.float64) - want_r) <= half_ulp + 1e-9).all(), q
            e32 = float(np.abs(got.astype(np.float64) - want_r).max())
            if admitted:
                assert e32 <= bound <= 1e-4, (q, px.shape, e32, bound)
            else:
                assert np.array_equal(got, got64), q


def _at_low_word(buf, low, nbytes, at=0):
    """A 256-B aligned slice of `buf` (uint8, > 4 GiB) starting `at` bytes past the first
    address whose low 32 bits are >= `low` (running past 2^32 if it is long enough)."""
    off = (low - buf.data_ptr()) % (1 << 32)
    off = (off + 255) // 256 * 256 + at
    assert off + nbytes <= buf.numel()
    return buf[off:off + nbytes]


@pytest.mark.parametrize("low", [0x80000000, 0xFFFF0000])
def test_outputs_at_addresses_with_bit31(T, dm, low):
    """Outputs placed where the device address's low word has bit 31 set (0x80000000..)
    or runs over a 4 GiB line (0xFFFF0000..): the paired-lane kernels' stores (store_stage:
    round trip recon, dctq_inverse, dctq_forward_float) and the coefficient stores must
    land exactly where the same launch writes into an ordinary allocation.  The round-5
    device faults came from store_stage sign-extending the low half of its readfirstlane'd
    base address (profiles/r05/INDEX.md)."""
    luma = dm.synth(4242, "uniform", 1920, 1080, 2)
    chroma = dm.synth(4343, "uniform", 960, 536, 4)
    nb = [px.shape[0] * (px.shape[1] // 8) * (px.shape[2] // 8) for px in (luma, chroma)]
    buf = T.empty((1 << 32) + (64 << 20), dtype=T.uint8, device="cuda")
    for q, ad in [(50, 0), (50, 1)]:
        plan = dm.Plan(q, ad)
        (c0, c1), (r0, r1) = plan.round_trip_planes([luma, chroma])
        at = [0, 9 << 20, 16 << 20, 34 << 20]  # co[0], co[1], re[0], re[1]: disjoint, inside 64 MiB
        co = [_at_low_word(buf, low, n * 128, a).view(T.int16).view(n, 64) for a, n in zip(at[:2], nb)]
        re = [_at_low_word(buf, low, n * 256, a).view(T.float32).view(n, 64) for a, n in zip(at[2:], nb)]
        plan.round_trip_planes([luma, chroma], outs=co, recons=re)
        assert T.equal(co[0], c0) and T.equal(co[1], c1), (q, ad)
        assert T.equal(re[0], r0) and T.equal(re[1], r1), (q, ad)
        vn = T.empty(nb[0], dtype=T.int32, device="cuda")
        plan.forward_quant(luma, var_num=vn)
        want = plan.inverse(c0, var_num=vn)
        got = _at_low_word(buf, low, nb[0] * 256).view(T.float32).view(nb[0], 64)
        plan.inverse(c0, var_num=vn, out=got)
        assert T.equal(got, want), (q, ad)
        wf = plan.forward_float(luma)
        gf = _at_low_word(buf, low, nb[0] * 256, 16 << 20).view(T.float32).view(nb[0], 64)
        plan.forward_float(luma, out=gf)
        assert T.equal(gf, wf), (q, ad)
        gq = _at_low_word(buf, low, nb[0] * 128).view(T.int16).view(nb[0], 64)
        plan.forward_quant(luma, out=gq)
        assert T.equal(gq, c0), (q, ad)
    del buf
    T.cuda.empty_cache()


def test_round_trip_exact_count_matches_forward(T, dm):
    """The fused kernel resolves ties in place; it recomputes exactly the
    coefficients the forward kernel sends to its deferred queue."""
    rng = np.random.default_rng(8)
    px = gpu_px(T, _step_blocks(rng, 48, 96))
    counts = []
    for fused in (False, True):
        plan = dm.Plan(50, 0)
        cnt = T.zeros(1, dtype=T.int64, device="cuda")
        plan.set_fallback_counter(cnt)
        if fused:
            plan.round_trip_planes([px])
        else:
            plan.forward_quant(px)
        T.cuda.synchronize()
        counts.append(int(cnt.item()))
        plan.set_fallback_counter(None)
    assert counts[0] == counts[1] and counts[0] > 100, counts


def test_example_block_pipeline(T, dm, blocks):
    """tests/test_entropy.c:290-393 example block through the batched API."""
    from golden.make_golden import EXAMPLE
    px = EXAMPLE.reshape(8, 8)
    for q in QUALITIES:
        for ad in (0, 1):
            plan = dm.Plan(q, ad)
            vn = T.zeros(1, dtype=T.int32, device="cuda")
            coef = plan.forward_quant(gpu_px(T, px), var_num=vn)
            assert coef.cpu().numpy().ravel().tolist() == blocks[f"example_q{q}_a{ad}"]
            rec = plan.inverse(coef, var_num=vn).cpu().numpy().astype(np.float64).ravel()
            want = f64(blocks[f"example_recon{q}_a{ad}"]) + 128.0
            assert np.abs(rec - want).max() <= 1e-4
    got = dm.Plan(50, 0).forward_float(gpu_px(T, px)).cpu().numpy().ravel()
    assert np.abs(got - f64(blocks["example_forward"])).max() <= 1e-4


def test_invalid_arguments(T, dm):
    import torch
    plan = dm.Plan(50, 0)
    with pytest.raises(dm.DctqError):
        plan.forward_quant(torch.zeros((12, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(dm.DctqError):
        plan.forward_quant(torch.zeros((16, 16), dtype=torch.uint8, device="cuda")[:, 1:9])
    with pytest.raises(dm.DctqError):
        dm.Plan(50, 1).inverse(torch.zeros((4, 64), dtype=torch.int16, device="cuda"))
    # the multi-plane calls: 0 or 5 planes, a bad plane among good ones, NULL outputs
    g = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    for fn in (plan.round_trip_planes, plan.encode_planes, plan.huffman_bits_planes):
        with pytest.raises(dm.DctqError):
            fn([g] * 5)
        with pytest.raises(dm.DctqError):
            fn([g, torch.zeros((12, 16), dtype=torch.uint8, device="cuda")])
    L = dm.lib()
    d = (dm._Plane * 1)(dm.plane_desc(g))
    o = torch.empty((4, 64), dtype=torch.int16, device="cuda")
    cp = C.cast((C.c_void_p * 1)(o.data_ptr()), C.c_void_p)
    assert L.dctq_round_trip_planes(plan._h, d, 1, cp, None, None, None) != 0           # recon array NULL
    off = torch.empty(5, dtype=torch.int32, device="cuda")
    assert L.dctq_encode_planes(plan._h, d, 1, cp, C.c_void_p(off.data_ptr()), None, 0, None, None) != 0  # no ws
    assert L.dctq_encode_planes(plan._h, d, 1, cp, C.c_void_p(off.data_ptr()), None, -1, C.c_void_p(off.data_ptr()),
                                None) != 0                                                 # negative capacity
    assert L.dctq_huffman_bits_planes(plan._h, d, 1, None, None) != 0                     # bits NULL
    assert L.dctq_huffman_bits_planes(plan._h, d, 1, C.c_void_p(off.data_ptr() + 2), None) != 0  # misaligned
    assert L.dctq_huffman_bits_planes(None, d, 1, C.c_void_p(off.data_ptr()), None) != 0  # no plan
    # a workspace is 4-byte aligned (include/dct_amd.h): workspace + 1 and + 2 are refused, nothing is launched
    ws = torch.empty(int(L.dctq_encode_workspace_bytes(4)) // 4 + 2, dtype=torch.int32, device="cuda")
    sym = torch.empty(4 * 64, dtype=torch.int32, device="cuda")
    for fn, name in ((L.dctq_encode_planes, "dctq_encode_planes"), (L.dctq_encode_planes16, "dctq_encode_planes16")):
        for delta in (1, 2):
            off.fill_(-7)
            o.fill_(-7)
            assert fn(plan._h, d, 1, cp, C.c_void_p(off.data_ptr()), C.c_void_p(sym.data_ptr()), 4 * 64,
                      C.c_void_p(ws.data_ptr() + delta), None) == -1, (name, delta)
            assert b"workspace" in L.dctq_error_string(-1), (name, delta)
            torch.cuda.synchronize()
            assert bool((off == -7).all()) and bool((o == -7).all()), (name, delta, "a refused call wrote")
        assert fn(plan._h, d, 1, cp, C.c_void_p(off.data_ptr()), C.c_void_p(sym.data_ptr()), 4 * 64,
                  C.c_void_p(ws.data_ptr()), None) == 0, name   # the same call, unrefused
        torch.cuda.synchronize()
        assert off.tolist() == [0, 2, 4, 6, 8], name  # four constant blocks: the DC and the closing symbol each
    wr = torch.empty(int(L.dctq_rle_workspace_bytes(4)) // 4 + 2, dtype=torch.int32, device="cuda")
    o.zero_()
    for delta in (1, 2):
        off.fill_(-7)
        assert L.dctq_rle_count(C.c_void_p(o.data_ptr()), 4, C.c_void_p(off.data_ptr()), C.c_void_p(wr.data_ptr() + delta),
                                None) == -1, delta
        torch.cuda.synchronize()
        assert bool((off == -7).all()), (delta, "a refused dctq_rle_count wrote offsets")
    assert L.dctq_rle_count(C.c_void_p(o.data_ptr()), 4, C.c_void_p(off.data_ptr()), C.c_void_p(wr.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert off.tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------ legacy per-block API
class DCTContext(C.Structure):
    _fields_ = [("block_size", C.c_int), ("dct_matrix", C.POINTER(C.POINTER(C.c_double))),
                ("transposed_dct", C.POINTER(C.POINTER(C.c_double)))]


class QuantContext(C.Structure):
    _fields_ = [("block_size", C.c_int), ("quality", C.c_int), ("quant_matrix", C.POINTER(C.POINTER(C.c_double))),
                ("dequant_matrix", C.POINTER(C.POINTER(C.c_double))), ("adaptive", C.c_int)]


@pytest.fixture(scope="module")
def L(T, dm):
    lib = dm.lib()
    P2 = C.POINTER(C.POINTER(C.c_double))
    I2 = C.POINTER(C.POINTER(C.c_int))
    lib.dct_init.restype = C.POINTER(DCTContext)
    lib.dct_forward.argtypes = [C.POINTER(DCTContext), P2, P2]
    lib.dct_inverse.argtypes = [C.POINTER(DCTContext), P2, P2]
    lib.alloc_array.restype = P2
    lib.alloc_int_array.restype = I2
    lib.free_array.argtypes = [P2, C.c_int]
    lib.free_int_array.argtypes = [I2, C.c_int]
    lib.quant_init.restype = C.POINTER(QuantContext)
    lib.quantize.argtypes = [C.POINTER(QuantContext), P2, I2, C.c_double]
    lib.dequantize.argtypes = [C.POINTER(QuantContext), I2, P2, C.c_double]
    lib.calculate_block_variance.argtypes = [P2, C.c_int]
    lib.calculate_block_variance.restype = C.c_double
    lib.adjust_matrix_for_block.argtypes = [C.POINTER(QuantContext), C.c_double, C.c_int]
    lib.adjust_matrix_for_block.restype = P2
    lib.copy_block_to_coefficients.argtypes = [P2, I2, C.c_int]
    lib.create_block_from_pixels.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.create_block_from_pixels.restype = P2
    lib.dct_free.argtypes = [C.POINTER(DCTContext)]
    lib.quant_free.argtypes = [C.POINTER(QuantContext)]
    return lib


def _put(L, a):
    n = a.shape[0]
    m = L.alloc_array(n, n)
    for i in range(n):
        for j in range(n):
            m[i][j] = float(a[i, j])
    return m


def _get(m, n):
    return np.array([[m[i][j] for j in range(n)] for i in range(n)])


def _put_i(L, a):
    n = a.shape[0]
    m = L.alloc_int_array(n, n)
    for i in range(n):
        for j in range(n):
            m[i][j] = int(a[i, j])
    return m


def _get_i(m, n):
    return np.array([[m[i][j] for j in range(n)] for i in range(n)], np.int64)


def test_legacy_transforms_bit_exact(L, blocks):
    from golden.make_golden import EXAMPLE
    ctx = L.dct_init(8)
    assert (_get(ctx.contents.dct_matrix, 8).ravel().view(np.uint64) == np.array(blocks["dct8"], np.uint64)).all()
    x = EXAMPLE.reshape(8, 8).astype(np.float64) - 128.0
    a, b = _put(L, x), L.alloc_array(8, 8)
    L.dct_forward(ctx, a, b)
    got = _get(b, 8).ravel()
    assert (got.view(np.uint64) == np.array(blocks["example_forward"], np.uint64)).all()
    c = L.alloc_array(8, 8)
    L.dct_inverse(ctx, b, c)
    assert (_get(c, 8).ravel().view(np.uint64) == np.array(blocks["example_inverse_of_forward"], np.uint64)).all()
    for m in (a, b, c):
        L.free_array(m, 8)
    L.dct_free(ctx)
    for n in (4, 16):
        ctx = L.dct_init(n)
        xin = np.array(blocks[f"blk{n}_in"], np.float64).reshape(n, n)
        a, b = _put(L, xin), L.alloc_array(n, n)
        L.dct_forward(ctx, a, b)
        assert (_get(b, n).ravel().view(np.uint64) == np.array(blocks[f"blk{n}_forward"], np.uint64)).all()
        L.dct_inverse(ctx, a, b)
        assert (_get(b, n).ravel().view(np.uint64) == np.array(blocks[f"blk{n}_inverse"], np.uint64)).all()
        L.free_array(a, n)
        L.free_array(b, n)
        L.dct_free(ctx)


def test_legacy_thread_churn(T, dm):
    """The per-block API from threads that come and go (legacy.hip lanes): 4 rounds of 6 concurrent
    Python threads (each an OS thread; ctypes drops the GIL inside the calls), each running
    dct_forward -> calculate_block_variance -> quantize on its own blocks over ONE shared context,
    n = 8 (zero-copy staging) and n = 40 (device scratch).  Every result equals the oracle's, and
    the lanes are reused: a thread that exits returns its lane to the pool, so 24 threads over 4
    rounds create at most 6 lanes (+ this thread's), with the rest pooled at the end.  Calls go
    through the diagnostic library, which exports the same API and counts its lanes."""
    import threading
    import oracle as O
    lib = dm.diag()
    P2 = C.POINTER(C.POINTER(C.c_double))
    I2 = C.POINTER(C.POINTER(C.c_int))
    lib.dct_init.restype = C.POINTER(DCTContext)
    lib.dct_forward.argtypes = [C.POINTER(DCTContext), P2, P2]
    lib.alloc_array.restype = P2
    lib.alloc_int_array.restype = I2
    lib.free_array.argtypes = [P2, C.c_int]
    lib.free_int_array.argtypes = [I2, C.c_int]
    lib.quant_init.restype = C.POINTER(QuantContext)
    lib.quantize.argtypes = [C.POINTER(QuantContext), P2, I2, C.c_double]
    lib.calculate_block_variance.argtypes = [P2, C.c_int]
    lib.calculate_block_variance.restype = C.c_double
    made0, pooled0 = C.c_int(), C.c_int()
    dm._check(lib.dctq_diag_legacy_lanes(C.byref(made0), C.byref(pooled0)), lib)
    ctxs = {n: (lib.dct_init(n), lib.quant_init(n, 75, 1)) for n in (8, 40)}
    rng = np.random.default_rng(606)
    errs = []

    def work(seed):
        try:
            r = np.random.default_rng(seed)
            for n in (8, 40, 8):
                dct, qc = ctxs[n]
                x = r.integers(-128, 128, (n, n)).astype(np.float64)
                a, c, q = _put(lib, x), lib.alloc_array(n, n), lib.alloc_int_array(n, n)
                lib.dct_forward(dct, a, c)
                var = lib.calculate_block_variance(a, n)
                lib.quantize(qc, c, q, var)
                want_c = O.forward(x)
                assert (_get(c, n).view(np.uint64) == want_c.view(np.uint64)).all(), (seed, n)
                assert var == O.variance(x), (seed, n)
                assert np.array_equal(_get_i(q, n), O.quantize(want_c, 75, 1, O.variance(x))), (seed, n)
                lib.free_array(a, n)
                lib.free_array(c, n)
                lib.free_int_array(q, n)
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs.append(repr(e))

    import time
    made, pooled = C.c_int(), C.c_int()
    for rnd in range(4):
        th = [threading.Thread(target=work, args=(int(rng.integers(1 << 30)),)) for _ in range(6)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not errs, errs
        # Python's join returns before the OS thread has run its thread_local destructors (which
        # hand the lanes back): wait for them before the next round starts its threads
        t_end = time.time() + 10
        while True:
            dm._check(lib.dctq_diag_legacy_lanes(C.byref(made), C.byref(pooled)), lib)
            if pooled.value >= pooled0.value + 6 or time.time() > t_end:
                break
            time.sleep(0.01)
    assert made.value - made0.value <= 6, (made0.value, made.value)
    assert pooled.value == pooled0.value + 6 and pooled.value <= made.value, (pooled0.value, pooled.value, made.value)


def test_legacy_large_blocks_and_variance(L):
    """The per-block API on both sides of the legacy kernels' staging switch (4 n^2 doubles up to 32 KiB:
    one workgroup with D, T and the block in LDS over the zero-copy buffer; above: device scratch and one
    launch per pass), against the oracle's restatement (bit-exact doubles); the variance of the same blocks
    (reference order)."""
    import oracle as O
    rng = np.random.default_rng(77)
    for n in (31, 32, 33, 45, 64, 65):
        ctx = L.dct_init(n)
        x = rng.integers(-128, 128, (n, n)).astype(np.float64) + rng.random((n, n))
        a, b, c = _put(L, x), L.alloc_array(n, n), L.alloc_array(n, n)
        L.dct_forward(ctx, a, b)
        assert (_get(b, n).view(np.uint64) == O.forward(x).view(np.uint64)).all(), n
        L.dct_inverse(ctx, b, c)
        assert (_get(c, n).view(np.uint64) == O.inverse(O.forward(x)).view(np.uint64)).all(), n
        v = L.calculate_block_variance(a, n)
        assert np.float64(v).view(np.uint64) == np.float64(O.variance(x)).view(np.uint64), n
        for m in (a, b, c):
            L.free_array(m, n)
        L.dct_free(ctx)


def _set_table(m, a):
    n = a.shape[0]
    for i in range(n):
        for j in range(n):
            m[i][j] = float(a[i, j])


def test_legacy_public_tables_and_large_n(L):
    """dct_forward / dct_inverse read the context's PUBLIC tables
    as the caller holds them (transposed_dct in the first pass, src/dct.c:61,89;
    dct_matrix in the second), for any block size the reference accepts (dct_init
    takes any n, src/dct.c:7-40) -- bit-exact against digests of the compiled
    reference's own outputs (tests/golden/legacy_tables.json); the variance of the
    large blocks against the oracle."""
    import hashlib
    import json
    import sys
    import oracle as O
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_legacy_golden import case_inputs
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "legacy_tables.json")))
    for c in g["cases"]:
        n = c["n"]
        x, d, t = case_inputs(n, c["seed"], c["edit"])
        ctx = L.dct_init(n)
        if c["edit"] is None:
            assert (_get(ctx.contents.dct_matrix, n).view(np.uint64) == d.view(np.uint64)).all(), c["name"]
        else:
            _set_table(ctx.contents.dct_matrix, d)
            _set_table(ctx.contents.transposed_dct, t)
        a, b, e = _put(L, x), L.alloc_array(n, n), L.alloc_array(n, n)
        L.dct_forward(ctx, a, b)
        fw = _get(b, n)
        assert hashlib.sha256(fw.tobytes()).hexdigest() == c["forward_sha256"], c["name"]
        L.dct_inverse(ctx, b, e)
        assert hashlib.sha256(_get(e, n).tobytes()).hexdigest() == c["inverse_of_forward_sha256"], c["name"]
        if c["edit"] is None and n > 64:
            v = L.calculate_block_variance(a, n)
            assert np.float64(v).view(np.uint64) == np.float64(O.variance(x)).view(np.uint64), n
        for m in (a, b, e):
            L.free_array(m, n)
        L.dct_free(ctx)


def test_legacy_quantization_bit_exact(L, blocks):
    from golden.make_golden import EXAMPLE
    c = f64(blocks["example_forward"]).reshape(8, 8)
    var = blocks["example_variance"]
    px = (C.c_char * 64).from_buffer_copy(EXAMPLE.tobytes())
    blk = L.create_block_from_pixels(px, 8, 0, 0, 8)
    assert L.calculate_block_variance(blk, 8) == var
    for q in QUALITIES:
        for ad in (0, 1):
            ctx = L.quant_init(8, q, ad)
            cm, qm = _put(L, c), L.alloc_int_array(8, 8)
            L.quantize(ctx, cm, qm, var)
            assert _get_i(qm, 8).ravel().tolist() == blocks[f"example_q{q}_a{ad}"]
            dq = L.alloc_array(8, 8)
            L.dequantize(ctx, qm, dq, var)
            assert (_get(dq, 8).ravel().view(np.uint64) == np.array(blocks[f"example_dq{q}_a{ad}"], np.uint64)).all()
            L.free_array(cm, 8)
            L.free_array(dq, 8)
            L.free_int_array(qm, 8)
            L.quant_free(ctx)
    ctx = L.quant_init(8, 50, 1)
    for vv in (0.0, 8.02, 99.5, 500.0, 864.2, 1000.0, 5000.0):
        for isq in (0, 1):
            m = L.adjust_matrix_for_block(ctx, vv, isq)
            assert (_get(m, 8).ravel().view(np.uint64) == np.array(blocks[f"adjust_50_{vv}_{isq}"], np.uint64)).all()
            L.free_array(m, 8)
    L.quant_free(ctx)
    cm, im = _put(L, c), L.alloc_int_array(8, 8)
    L.copy_block_to_coefficients(cm, im, 8)
    assert _get_i(im, 8).ravel().tolist() == blocks["example_round"]


def test_c_host_programs(T, dm, blocks, tmp_path):
    """The C hosts in host/ (linked against libdct_amd.so through include/*.h)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["make", "-C", os.path.join(root, "host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    r = subprocess.run([os.path.join(root, "host", "block_pipeline")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(l.split(":", 1) for l in r.stdout.strip().splitlines() if ":" in l)
    assert [int(v) for v in lines["q50"].split()] == blocks["example_q50_a0"]
    assert [int(v) for v in lines["q90"].split()] == blocks["example_q90_a0"]
    assert int(lines["forward_bits0"], 16) == blocks["example_forward"][0]
    import oracle as O
    for (w, h, q, ad, kind) in [(1920, 1080, 50, 0, 0), (640, 480, 90, 1, 1)]:
        r = subprocess.run([os.path.join(root, "host", "frame_codec"), str(w), str(h), str(q), str(ad), "12345",
                            str(kind)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = dict(l.split(":", 1) for l in r.stdout.strip().splitlines())
        want = O.forward_plane(O.synth_plane(12345, kind, w, h), q, ad).tobytes()
        fnv = 1469598103934665603
        for b in want:
            fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert int(got["fnv1a"], 16) == fnv, (w, h, q, ad)
        assert got["fused"] == "ok", (w, h, q, ad)
        _, wsym = O.rle_encode_plane(np.frombuffer(want, np.int16).reshape(-1, 64))
        fs = 1469598103934665603
        for b in wsym.tobytes():
            fs = ((fs ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert int(got["symbols"]) == wsym.size and int(got["symbols_fnv1a"], 16) == fs, (w, h, q, ad)
        assert int(got["symbol_bytes"]) == dm.symbol_bytes(q, ad) == 2, (w, h, q, ad)
        # the default entry point keeps the 4-byte format for every plan (ABI 6)
        assert got["symbols4_equal"] == "1" and int(got["abi_version"]) == 6, got
        want_bits = int(O.huffman_bits_plane(np.frombuffer(want, np.int16).reshape(-1, 64)).astype(np.uint64).sum())
        assert int(got["huffman_bits"]) == want_bits, (w, h, q, ad)


def _run_mt(root, pxfile, w, h, q, ad, threads, reps, out):
    import subprocess
    r = subprocess.run([os.path.join(root, "host", "block_pipeline_mt"), str(pxfile), str(w), str(h), str(q), str(ad),
                        str(threads), str(reps), str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    return dict(l.split(":", 1) for l in r.stdout.strip().splitlines())


def test_legacy_threads_overlap(T, dm, tmp_path):
    """the per-block drop-in from 8 host threads over ONE shared
    DCTContext / QuantContext (host/block_pipeline_mt.c: the 5-call pipeline of
    host/block_pipeline.c per block).  Each thread has its own stream and staging
    buffer (legacy.hip lanes) and takes no lock after its first call: bit-exact
    quantized ints and reconstructions (oracle), identical to one thread, >= 3x the
    one-thread pipeline rate, and glibc's seed-1 rand() sequence drawn by the main
    thread while the workers run is undisturbed."""
    import subprocess
    import oracle as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["make", "-C", os.path.join(root, "host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    w, h, q, ad = 256, 128, 50, 1
    px = O.synth_plane(4321, O.KINDS["smooth"], w, h)
    pxfile = tmp_path / "px.u8"
    px.tofile(pxfile)
    rec = np.dtype([("q", "<i4", 64), ("r", "<f8", 64)])
    want_q = O.forward_plane(px, q, ad).astype(np.int32)
    want_r = O.inverse_plane(want_q, q, ad, O.plane_variance(px))
    res = {}
    for threads in (1, 8):
        f = tmp_path / f"out{threads}.bin"
        res[threads] = _run_mt(root, pxfile, w, h, q, ad, threads, 3, f)
        got = np.fromfile(f, rec)
        assert np.array_equal(got["q"], want_q), threads
        assert np.array_equal(got["r"].view(np.uint64), want_r.view(np.uint64)), threads  # bit-exact doubles
        assert res[threads]["rand_ok"] == "1", res[threads]
    assert (tmp_path / "out1.bin").read_bytes() == (tmp_path / "out8.bin").read_bytes()
    assert int(res[8]["rand_draws"]) > 1000, res[8]
    r1, r8 = float(res[1]["pipelines_per_s"]), float(res[8]["pipelines_per_s"])
    print(f"legacy per-block pipeline: 1 thread {r1:.0f}/s, 8 threads {r8:.0f}/s ({r8 / r1:.2f}x)")
    assert r8 >= 3.0 * r1, (r1, r8)


@pytest.mark.parametrize("prog", ["dct", "quantization", "entropy"])
def test_reference_programs_relinked(T, dm, prog):
    """Drop-in check: the reference's OWN test programs (tests/test_<prog>.c, with
    the reference's headers), linked against libdct_amd.so in place of
    src/{utils,dct,quantization}.c, print exactly what they print when linked
    against the reference (tests/golden/ref_programs.json) and exit 0.  The
    binaries are built by oracle/Makefile where /root/reference exists and
    travel to the GPU box as built files (oracle/_ref/)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", f"test_{prog}_amd")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_*_amd not built (needs /root/reference at build time)")
    want = json.load(open(os.path.join(root, "tests", "golden", "ref_programs.json")))[prog]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == want["rc"], r.stderr
    assert r.stdout == want["stdout"]


def test_rle_bit_exact_and_round_trip(T, dm):
    """Zigzag + RLE on the GPU (src/entropy.c:158-256 per block) == the oracle
    (pinned to the reference's entropy.c by tests/golden/rle.json), and the GPU
    decode restores every block (run_length_decode, :327-351)."""
    import json
    import oracle as O
    root = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(root, "golden", "rle.json")))
    golden = np.array([b["coeffs"] for b in g["blocks"].values()], np.int16)
    rng = np.random.default_rng(11)
    cases = [golden, np.zeros((5, 64), np.int16), np.full((3, 64), 7, np.int16),
             (rng.integers(-600, 600, (1000, 64)) * (rng.random((1000, 64)) < 0.15)).astype(np.int16)]
    px = O.synth_plane(4, O.KINDS["smooth"], 640, 480)
    cases.append(O.forward_plane(px, 75, 0))          # real quantized planes: ragged tiles (4800 blocks)
    cases.append(O.forward_plane(O.synth_plane(5, 0, 512, 256), 90, 1))

    def blocks_with(counts):  # block i has counts[i] symbols: counts[i]-1 nonzeros off (7,7), (7,7) zero
        b = np.zeros((len(counts), 64), np.int16)
        for i, k in enumerate(counts):
            b[i, rng.permutation(63)[:k - 1]] = rng.integers(1, 300, k - 1) * rng.choice([-1, 1], k - 1)
        return b
    # emit's two paths (rle.hip): tiles of <= 2048 symbols go lane-per-block through LDS (flushed in
    # rounds of 1024), denser ones wave-per-block -- tiles at 1024 / 1025 and 2048 / 2049 symbols,
    # alternating tiles, a ragged sparse tail;
    # decode's: half tiles (32 blocks) of <= 240 symbols lane path, <= 1024 walk path, denser scan path --
    # halves at 240 / 241 and 1024 / 1025 symbols, and walk halves with 64-symbol blocks
    cases.append(blocks_with([16] * 64 + [16] * 63 + [17] + [1] * 64 + [64] * 64 + [2] * 64 + [40] * 64
                             + [7] * 16 + [8] * 16 + [7] * 15 + [8] * 17 + [32] * 32 + [32] * 31 + [33]
                             + [64] * 8 + [1] * 24 + [32] * 64 + [32] * 63 + [33] + [3] * 29))
    for c in cases:
        off, sym = dm.rle_encode(T.from_numpy(c).cuda())
        woff, wsym = O.rle_encode_plane(c)
        assert np.array_equal(off.cpu().numpy().view(np.uint32), woff)
        assert np.array_equal(sym.cpu().numpy().view(np.uint32), wsym)
        back = dm.rle_decode(sym, off).cpu().numpy()
        assert np.array_equal(back, c)
        if np.abs(c).max(initial=0) <= 511:  # the 2-byte format (dctq_rle_decode16): every decode path,
            s16 = T.from_numpy(O.pack16(wsym).view(np.int16).copy()).cuda()  # odd half / lane starts
            assert np.array_equal(dm.rle_decode(s16, off).cpu().numpy(), c)
    for name, b in g["blocks"].items():  # the reference's own symbols, block by block
        off, sym = dm.rle_encode(T.from_numpy(np.array([b["coeffs"]], np.int16)).cuda())
        s = sym.cpu().numpy().view(np.uint32)
        assert ((s & 0xFFFF).astype(np.uint16).view(np.int16).tolist(), (s >> 16).tolist()) == \
            (b["values"], b["runs"]), name


def test_rle_large_planes(T, dm):
    """Block counts past one tile-scan chunk (8192 tiles = 524 288 blocks) and
    with a ragged last tile: 5 4K luma frames plus 37 blocks, several tiles per
    wave in the count pass, every offset and symbol against the oracle."""
    import oracle as O
    px = dm.synth(31, "uniform", 3840, 2160, 5)
    coef = dm.Plan(50, 0).forward_quant(px)
    extra = T.from_numpy(O.forward_plane(O.synth_plane(32, 1, 8 * 37, 8), 50, 0)).cuda()
    c = T.cat([coef, extra]).contiguous()
    off, sym = dm.rle_encode(c)
    woff, wsym = O.rle_encode_plane(c.cpu().numpy())
    assert np.array_equal(off.cpu().numpy().view(np.uint32), woff)
    assert np.array_equal(sym.cpu().numpy().view(np.uint32), wsym)
    assert np.array_equal(dm.rle_decode(sym, off).cpu().numpy(), c.cpu().numpy())
    s16 = T.from_numpy(O.pack16(wsym).view(np.int16).copy()).cuda()
    assert np.array_equal(dm.rle_decode(s16, off).cpu().numpy(), c.cpu().numpy())


def test_huffman_bits_golden_and_planes(T, dm):
    """Per-block Huffman size on the GPU (huffman.hip: sort network + frequency histogram +
    bucket merge) == the reference's get_encoded_size after build_huffman_codes
    (tests/golden/huffman.json, made by the compiled reference) and == the oracle's literal
    heap restatement on quantized planes of every input kind, ragged tile counts included."""
    import json
    import oracle as O
    root = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(root, "golden", "huffman.json")))
    golden = np.array([b["coeffs"] for b in g["blocks"].values()], np.int16)
    got = dm.huffman_bits(T.from_numpy(golden).cuda()).cpu().numpy().view(np.uint32)
    assert got.tolist() == [b["bits"] for b in g["blocks"].values()]
    rng = np.random.default_rng(21)
    cases = [np.zeros((1, 64), np.int16), np.full((65, 64), -3, np.int16),
             (rng.integers(-1024, 1025, (777, 64)) * (rng.random((777, 64)) < 0.5)).astype(np.int16)]
    # one tile per path of the kernel (every block <= 16 / <= 32 / some > 32 nonzero coefficients), with
    # nonzeros at random positions (c[63] zero or not) and few distinct values (long runs, ties)
    for lo, hi in [(0, 16), (17, 32), (30, 40), (16, 17), (32, 33)]:
        blk = np.zeros((64, 64), np.int16)
        for r in range(64):
            k = int(rng.integers(lo, hi + 1))
            blk[r, rng.choice(64, k, replace=False)] = rng.choice([-3, -1, 1, 2, 5, 300], k)
        cases.append(blk)
    # the counting path of dense tiles (every block's values, zeros included, span < 64 integers): a span
    # of exactly 63, a window clear of zero (no zeros), one value 64 times; the same tile with one block
    # spanning 64 takes the sort path
    blk = np.zeros((64, 64), np.int16)
    for r in range(64):
        k = int(rng.integers(33, 65))
        blk[r, rng.choice(64, k, replace=False)] = rng.integers(-31, 33, k)
    blk[0] = np.arange(-31, 33)
    blk[1] = -100 + np.arange(64)
    blk[2] = 5
    cases.append(blk)
    wide = blk.copy()
    wide[3, 7] = 64
    cases.append(wide)
    for kind, q, ad in [("uniform", 50, 0), ("smooth", 90, 1), ("const", 10, 0), ("extreme", 100, 0),
                        ("uniform", 1, 1)]:
        cases.append(O.forward_plane(O.synth_plane(7, O.KINDS[kind], 8 * 61, 8 * 9), q, ad))  # 549 blocks
    for c in cases:
        got = dm.huffman_bits(T.from_numpy(c).cuda()).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, O.huffman_bits_plane(c))


def test_huffman_bits_frequency_shapes(T, dm):
    """The register merge on the shapes its closed form and masks must handle, through every path:
    blocks built from frequency partitions (tests/test_oracle.py::register_merge_wpl's generator)
    -- light leaves only, one to three leaves heavier than 16 (the weight rows read with the light
    ones, 17..20, and the rows read one by one, 21..64), pending merges above 16 -- laid out as
    dense tiles of span < 64 (the narrow counting path), as <= 32-nonzero tiles (the sparse sort
    paths) and as wide dense tiles (the 64-network), each block against the oracle."""
    import oracle as O
    rng = np.random.default_rng(2024)

    def partition(total, heavy):
        f = list(heavy)
        left = total - sum(f)
        while left:
            x = int(min(left, rng.choice([1, 1, 2, 3, 4, 5, 8, 16])))
            f.append(x)
            left -= x
        return f

    def block(freqs, base, zeros_last):
        vals = [base + i for i, x in enumerate(freqs) for _ in range(x)]
        b = np.zeros(64, np.int16)
        pos = rng.permutation(63 if zeros_last else 64)[:len(vals)]
        b[pos] = vals
        return b

    heavies = [(), (17,), (20,), (21,), (30,), (17, 17), (20, 25), (17, 18, 19), (21, 21, 21), (40,), (64,),
               (33, 31), (18, 22, 23)]
    narrow, sparse, wide = [], [], []
    for r in range(64 * 6):
        h = heavies[r % len(heavies)]
        total = 64 if sum(h) < 64 or rng.random() < 0.5 else sum(h)
        f = partition(total, h)
        if len(f) > 63:
            f = f[:63]
        nb = block(f, int(rng.integers(-40, 2)), zeros_last=False)  # values in a window of <= 63: narrow
        nb[nb == 0] = 1 if (nb == 0).all() else nb[nb != 0][0]  # no zeros: the span stays that of the values
        narrow.append(nb)
        hs = [x for x in h if x <= 32][:1]
        fs = partition(int(rng.integers(sum(hs) if hs else 1, 33)), hs)
        sparse.append(block(fs, 1 + int(rng.integers(0, 50)), zeros_last=bool(rng.random() < 0.5)))
        w = block(f, -200, zeros_last=False)
        w[int(rng.integers(64))] = 300  # span > 64: the sort path
        wide.append(w)
    for c in (np.array(narrow), np.array(sparse), np.array(wide)):
        got = dm.huffman_bits(T.from_numpy(c).cuda()).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, O.huffman_bits_plane(c))


def test_huffman_bits_large_plane(T, dm):
    """A 4K luma frame stack (several tiles per wave in the grid-stride loop) + 5 ragged
    blocks, every block against the oracle; invalid arguments rejected."""
    import oracle as O
    coef = dm.Plan(75, 0).forward_quant(dm.synth(41, "smooth", 3840, 2160, 2))
    c = T.cat([coef, coef[:5]]).contiguous()
    got = dm.huffman_bits(c).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, O.huffman_bits_plane(c.cpu().numpy()))
    L = dm.lib()
    out = T.empty(8, dtype=T.int32, device="cuda")
    assert L.dctq_huffman_bits(None, 8, C.c_void_p(out.data_ptr()), None) == -1
    assert L.dctq_huffman_bits(C.c_void_p(c.data_ptr() + 2), 8, C.c_void_p(out.data_ptr()), None) == -1
    assert L.dctq_huffman_bits(C.c_void_p(c.data_ptr()), -1, C.c_void_p(out.data_ptr()), None) == -1
    assert L.dctq_huffman_bits(C.c_void_p(c.data_ptr()), 0, C.c_void_p(out.data_ptr()), None) == 0


def test_huffman_bits_tile_sequences(T, dm):
    """Many tiles per wave (20 011 tiles over the kernel's 8 192-wave grid): consecutive tiles
    of one wave take every pair of paths (narrow counting with the next tile's LDS-DMA in
    flight, 16/32-input sorts, the 64-network), and the last tile is ragged.  Every block
    against the oracle (computed once per distinct base tile)."""
    import oracle as O
    rng = np.random.default_rng(77)
    base = []
    for kind, q, ad in [("uniform", 50, 0), ("extreme", 10, 0), ("smooth", 90, 1), ("const", 50, 0),
                        ("uniform", 100, 0), ("smooth", 50, 0), ("extreme", 100, 1), ("uniform", 5, 0)]:
        plane = O.forward_plane(O.synth_plane(int(rng.integers(1 << 30)), O.KINDS[kind], 8 * 64, 8 * 4), q, ad)
        base += [plane[64 * k:64 * (k + 1)] for k in range(4)]
    wide = (rng.integers(-300, 301, (64, 64)) * (rng.random((64, 64)) < 0.8)).astype(np.int16)
    base.append(wide)  # dense, span >= 64: the sort network
    mid = np.zeros((64, 64), np.int16)  # 17..32 nonzero coefficients per block: the 32-input sort
    for r in range(64):
        k = int(rng.integers(17, 33))
        mid[r, rng.choice(64, k, replace=False)] = rng.integers(-40, 41, k) | 1
    base.append(mid)
    base = np.stack(base)
    want_base = np.stack([O.huffman_bits_plane(b) for b in base])
    order = rng.integers(0, len(base), 20011)
    nblk = 64 * (len(order) - 1) + 37
    coef = base[order].reshape(-1, 64)[:nblk]
    got = dm.huffman_bits(T.from_numpy(coef).cuda()).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want_base[order].reshape(-1)[:nblk])


def test_huffman_bits_planes_from_pixels(T, dm):
    """dctq_huffman_bits_planes (forward + quantization + per-block Huffman size in ONE launch,
    coefficients on chip) == dctq_huffman_bits over dctq_forward_quant_planes' output, bit-exact,
    blocks numbered plane by plane: every input kind, tie-heavy plans (extreme q10/q100, in-place
    exact resolution), adaptive plans, up to 4 planes of ragged geometry (partial last batches and
    tiles), and a stack large enough for many batches per wave.  One small plane also against the
    oracle's literal pipeline (forward_plane -> huffman_bits_plane)."""
    import oracle as O
    rng = np.random.default_rng(5)
    for kind, q, ad in [("uniform", 50, 0), ("extreme", 10, 0), ("smooth", 90, 1), ("const", 50, 0),
                        ("uniform", 100, 0), ("extreme", 100, 1), ("uniform", 1, 0), ("smooth", 75, 1)]:
        plan = dm.Plan(q, ad)
        planes = [dm.synth(int(rng.integers(1 << 30)), kind, 8 * 61, 8 * 9, 3),
                  dm.synth(int(rng.integers(1 << 30)), kind, 8 * 13, 8 * 5, 2),
                  dm.synth(int(rng.integers(1 << 30)), kind, 8 * 40, 8 * 8)]
        want = dm.huffman_bits(T.cat(plan.forward_quant_planes(planes)))
        got = plan.huffman_bits_planes(planes)
        T.cuda.synchronize()
        assert T.equal(got, want), (kind, q, ad)
    # against the oracle: one plane, the reference's pipeline restated
    px = O.synth_plane(11, O.KINDS["uniform"], 8 * 37, 8 * 11)
    want = O.huffman_bits_plane(O.forward_plane(px, 50, 0))
    got = dm.Plan(50, 0).huffman_bits_planes([gpu_px(T, px)]).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    # a 4K 4:2:0 stack
    plan = dm.Plan(50, 0)
    planes = [dm.synth(3, "uniform", 3840, 2160, 4), dm.synth(4, "uniform", 1920, 1080, 8)]
    want = dm.huffman_bits(T.cat(plan.forward_quant_planes(planes)))
    got = plan.huffman_bits_planes(planes)
    T.cuda.synchronize()
    assert T.equal(got, want)


def test_huffman_bits_planes_many_batches_per_wave(T, dm):
    """The fused kernel carries each next batch's rows in registers from one iteration to
    the next (loaded as soon as the tie pass is done with the current ones).  On the full
    grid a wave sees about one batch, so the plans here launch as if the device had 1-3
    CUs (dctq_diag_plan_set_num_cus): ~16-50 batches per wave, plane changes inside a
    wave's sequence, ragged planes with partial last batches, tie-heavy and adaptive plans.
    Reference: the two launches (forward_quant_planes -> huffman_bits), bit-exact."""
    rng = np.random.default_rng(12)
    for kind, q, ad, cus in [("uniform", 50, 0, 1), ("uniform", 50, 1, 2), ("extreme", 10, 0, 1),
                             ("smooth", 90, 0, 3), ("uniform", 100, 0, 1), ("extreme", 50, 1, 1)]:
        planes = [dm.synth(int(rng.integers(1 << 30)), kind, 3840, 2160),
                  dm.synth(int(rng.integers(1 << 30)), kind, 8 * 123, 8 * 67, 3),
                  dm.synth(int(rng.integers(1 << 30)), kind, 8 * 31, 8 * 7)]
        want = dm.huffman_bits(T.cat(dm.Plan(q, ad).forward_quant_planes(planes)))
        got = dm.Plan(q, ad, num_cus=cus).huffman_bits_planes(planes)
        T.cuda.synchronize()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (kind, q, ad, cus, bad[:8].flatten().tolist())
    # the same carry at a small shape: one workgroup (dct_amd.grid_limit), so 13 + 4 + 4 batches
    # of a 4:2:0 stack are five or six per wave, plane changes inside every wave's sequence
    planes = [dm.synth(51, "uniform", 136, 96, 4), dm.synth(52, "extreme", 72, 48, 4),
              dm.synth(53, "smooth", 72, 48, 4)]
    for q, ad in [(50, 0), (10, 1)]:
        want = dm.huffman_bits(T.cat(dm.Plan(q, ad).forward_quant_planes(planes)))
        with dm.grid_limit(1):
            got = dm.Plan(q, ad).huffman_bits_planes(planes)
            assert dm.last_grid() == 1
        T.cuda.synchronize()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (q, ad, "grid_limit(1)", bad[:8].flatten().tolist())


def test_encode_planes_fused(T, dm):
    """dctq_encode_planes (forward + zigzag/RLE, the count fused into the forward) equals the
    oracle's run_length_encode of the oracle's quantized planes, blocks numbered plane
    by plane: ragged planes, a frame stack, tie-heavy step blocks (ties resolved before
    counting: a tie can decide zero vs nonzero), adaptive plans."""
    import oracle as O
    rng = np.random.default_rng(44)
    stack = np.stack([O.synth_plane(90 + f, f % 4, 40, 24) for f in range(3)])
    sets = [[O.synth_plane(7, 0, 8 * 65, 8 * 9), _step_blocks(rng, 7, 13), O.synth_plane(8, 1, 8, 8), stack],
            [_step_blocks(rng, 21, 37)], [O.synth_plane(9, 3, 8 * 129, 8 * 3), O.synth_plane(10, 2, 64, 64)]]
    for q, ad in [(50, 0), (50, 1), (90, 0), (91, 0), (10, 1), (100, 0)]:
        plan = dm.Plan(q, ad)
        # 2-byte symbols exactly when the plan bounds every quantized coefficient by 511
        assert plan.symbol_bytes == (2 if q <= 90 else 4) == dm.symbol_bytes(q, ad), (q, ad)
        for planes in sets:
            want = np.concatenate([np.concatenate([O.forward_plane(f, q, ad) for f in (p if p.ndim == 3 else [p])])
                                   for p in planes])
            woff, wsym = O.rle_encode_plane(want)
            coefs, off, sym = plan.encode_planes([gpu_px(T, p) for p in planes])
            assert np.array_equal(T.cat(coefs).cpu().numpy(), want), (q, ad)
            assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), (q, ad)
            if plan.symbol_bytes == 2:
                assert sym.dtype == T.int16
                assert np.array_equal(sym.cpu().numpy().view(np.uint16), O.pack16(wsym)), (q, ad)
            else:
                assert np.array_equal(sym.cpu().numpy().view(np.uint32), wsym), (q, ad)
            # and back: the decoder of the stream's format restores every block
            assert np.array_equal(dm.rle_decode(sym, off).cpu().numpy(), want), (q, ad)
            # dctq_encode_planes writes the 4-byte format for EVERY plan (ABI 6);
            # the 2-byte format is dctq_encode_planes16, refused where values can exceed 511
            _, off4, sym4 = plan.encode_planes([gpu_px(T, p) for p in planes], symbol_bytes=4)
            assert sym4.dtype == T.int32 and np.array_equal(sym4.cpu().numpy().view(np.uint32), wsym), (q, ad)
            assert T.equal(off4, off)
            if plan.symbol_bytes == 4:
                with pytest.raises(dm.DctqError):
                    plan.encode_planes([gpu_px(T, p) for p in planes], symbol_bytes=2)
    assert dm.lib().dctq_abi_version() == 6


def test_encode_capacity_and_large(T, dm):
    """Symbols past the capacity are dropped while the offsets stay complete; and a
    multi-plane encode past one scan segment (5 4K frames + 1080p chroma) equals
    forward_quant_planes + rle_encode on the GPU."""
    import oracle as O
    plan = dm.Plan(50, 0)
    # dense and sparse tiles at q50, and q90 noise (~62 symbols per block: tiles near the 4 096 the
    # 2-byte lane-per-block path stages) -- every one through the emit's capacity cuts
    for q, kind in ((50, 0), (50, 1), (90, 0)):
        px = gpu_px(T, O.synth_plane(12, kind, 256, 128))
        plan = dm.Plan(q, 0)
        _, off, sym = plan.encode_planes([px])
        woff, wsym = O.rle_encode_plane(O.forward_plane(O.synth_plane(12, kind, 256, 128), q, 0))
        assert np.array_equal(off.cpu().numpy().view(np.uint32), woff) and np.array_equal(_sym32(sym), wsym), q
        total = int(off[-1].item())
        tile_end = int(off[64].item())
        for cap in (total // 3, total - 1, tile_end, tile_end + 1, 1):
            _, off2, sym2 = plan.encode_planes([px], capacity=cap)
            assert np.array_equal(off.cpu().numpy(), off2.cpu().numpy())
            assert sym2.numel() == cap and np.array_equal(sym2.cpu().numpy(), sym[:cap].cpu().numpy()), (kind, cap)
        # nothing at or past the capacity is written, in either format: the stream goes
        # into a LARGER buffer pre-filled with a sentinel, odd and even caps, tiles at odd offsets
        L = dm.lib()
        descs = (dm._Plane * 1)(dm.plane_desc(px))
        nb = px.shape[-1] // 8 * (px.shape[-2] // 8)
        coef = T.empty((nb, 64), dtype=T.int16, device="cuda")
        cp = (C.c_void_p * 1)(coef.data_ptr())
        offs = T.empty(nb + 1, dtype=T.int32, device="cuda")
        ws = T.empty(int(L.dctq_encode_workspace_bytes(nb)) // 4 + 1, dtype=T.int32, device="cuda")
        odd_tile = int(off[65].item())
        for sb, fn, dt in ((2, L.dctq_encode_planes16, T.int16), (4, L.dctq_encode_planes, T.int32)):
            full = (sym if sym.dtype == dt else plan.encode_planes([px], symbol_bytes=sb)[2]).cpu().numpy()
            for cap in (total // 3, total // 3 + 1, tile_end - 1, tile_end, tile_end + 1, odd_tile, odd_tile + 1,
                        total - 1, 1, 2, 3):
                buf = T.full((cap + 64,), 0x5A5A, dtype=dt, device="cuda")
                dm._check(fn(plan._h, descs, 1, C.cast(cp, C.c_void_p), C.c_void_p(offs.data_ptr()),
                             C.c_void_p(buf.data_ptr()), cap, C.c_void_p(ws.data_ptr()), None), L)
                T.cuda.synchronize()
                got = buf.cpu().numpy()
                assert np.array_equal(got[:cap], full[:cap]), (q, kind, sb, cap)
                assert (got[cap:] == 0x5A5A).all(), (q, kind, sb, cap, np.nonzero(got[cap:] != 0x5A5A)[0][:8])
    plan = dm.Plan(50, 0)
    luma = dm.synth(13, "uniform", 3840, 2160, 5)
    chroma = dm.synth(14, "smooth", 1920, 1080, 3)
    ecoefs, off, sym = plan.encode_planes([luma, chroma])
    coefs = plan.forward_quant_planes([luma, chroma])
    assert all(T.equal(a, b) for a, b in zip(ecoefs, coefs))
    woff, wsym = dm.rle_encode(T.cat(coefs).contiguous())
    assert T.equal(off, woff)
    assert sym.dtype == T.int16  # q50: 2-byte symbols
    assert np.array_equal(sym.cpu().numpy().view(np.uint16), O.pack16(wsym.cpu().numpy().view(np.uint32)))
    assert T.equal(dm.rle_decode(sym, off), T.cat(coefs))


def test_randomized_sweep_all_planes_apis(T, dm):
    """40 random configurations (kinds, qualities 1-100, adaptive, 1-4 planes of
    ragged geometry, frame stacks, padded rows) through forward_quant_planes,
    round_trip_planes and encode_planes, all against the oracle."""
    import oracle as O
    import torch
    rng = np.random.default_rng(2026)
    for trial in range(40):
        q = int(rng.integers(1, 101))
        ad = int(rng.integers(0, 2))
        nplanes = int(rng.integers(1, 5))
        planes, hosts = [], []
        for _ in range(nplanes):
            w, h = 8 * int(rng.integers(1, 48)), 8 * int(rng.integers(1, 24))
            nf = int(rng.integers(1, 4))
            pad = 8 * int(rng.integers(0, 3))
            kind = int(rng.integers(0, 4))
            frames = [O.synth_plane(int(rng.integers(1, 1 << 30)), kind, w, h) for _ in range(nf)]
            buf = torch.zeros((nf, h, w + pad), dtype=torch.uint8)
            for f in range(nf):
                buf[f, :, :w] = torch.from_numpy(frames[f])
            planes.append(buf.cuda()[:, :, :w])
            hosts.append(frames)
        plan = dm.Plan(q, ad)
        want = [np.concatenate([O.forward_plane(f, q, ad) for f in fr]) for fr in hosts]
        got = plan.forward_quant_planes(planes)
        for g, wv in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), wv), ("forward", trial, q, ad)
        coefs, recs = plan.round_trip_planes(planes)
        for c, r, wv, fr in zip(coefs, recs, want, hosts):
            assert np.array_equal(c.cpu().numpy(), wv), ("round trip", trial, q, ad)
            var = np.concatenate([O.plane_variance(f) for f in fr]) if ad else None
            ref = O.inverse_plane(wv, q, ad, var) + 128.0
            assert np.abs(r.cpu().numpy().astype(np.float64) - ref).max() <= 1e-4, ("recon", trial, q, ad)
        ecoefs, off, sym = plan.encode_planes(planes)
        woff, wsym = O.rle_encode_plane(np.concatenate(want))
        assert all(np.array_equal(c.cpu().numpy(), wv) for c, wv in zip(ecoefs, want)), ("encode coef", trial)
        assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), ("encode offsets", trial, q, ad)
        assert np.array_equal(_sym32(sym), wsym), ("encode symbols", trial, q, ad)


def test_every_dispatch_leaf(T, dm):
    """Every leaf of the launchers' bool dispatch (adaptive x var_num x fallback counter, the fp32 /
    fp64 inverse, decode8's three kernels, both adaptive settings of dctq_inverse, the encoder and
    the Huffman size from pixels), each against the oracle, on two planes in one call: 65 blocks
    (a full 64-block batch, a one-block tail, two full and a one-block 32-block batch) and 1 block
    (a plane switch).  Seeded uniform noise of a quarter of the u8 range: block variances of
    150-400, so an adaptive plan scales every block differently and never as a non-adaptive one
    (full-range noise has variance > 1000, where the adaptive divisor is Q again).  The DC keeps Q
    in every plan and is sum(px - 128) / (8 Q00): the blocks where that lies within 1e-9 of a half
    integer are inside every guard band (>= 2^-25 wide, fill_fast_tables), so the fallback counter
    must count them (tie flags of other coefficients on top)."""
    import oracle as O
    rng = np.random.default_rng(808)
    hosts = [rng.integers(96, 160, size=(40, 104), dtype=np.uint8), rng.integers(96, 160, size=(8, 8), dtype=np.uint8)]
    planes = [gpu_px(T, p) for p in hosts]
    shapes = [p.shape for p in hosts]
    var = [O.plane_variance(p) for p in hosts]
    sums = np.concatenate([p.astype(np.int64).reshape(h // 8, 8, w // 8, 8).sum(axis=(1, 3)).ravel() - 64 * 128
                           for p, (h, w) in zip(hosts, shapes)])
    q32, q64 = 50, 90
    assert dm.inverse_bound(q32, 0)[1] is True and dm.inverse_bound(q64, 0)[1] is False
    for q in (q32, q64):
        dc = np.abs(sums / 8.0 / O.quant_matrix(8, q)[0, 0])
        dc_ties = int((np.abs(dc - np.floor(dc) - 0.5) < 1e-9).sum())
        for ad in (0, 1):
            plan = dm.Plan(q, ad)
            want_c = [O.forward_plane(p, q, ad) for p in hosts]
            want_r = [O.inverse_plane(c, q, ad, v if ad else None) + 128.0 for c, v in zip(want_c, var)]
            if ad:
                assert not np.array_equal(want_c[0], O.forward_plane(hosts[0], q, 0))  # the leaves differ
            counts, recon = {}, None
            for with_var in (True, False):
                for with_cnt in (True, False):
                    cnt = T.zeros(1, dtype=T.int64, device="cuda")
                    plan.set_fallback_counter(cnt if with_cnt else None)
                    leaf = (q, ad, with_var, with_cnt)
                    for fused in (False, True):
                        vns = [T.full((p.size // 64,), -1, dtype=T.int32, device="cuda") for p in hosts] if with_var else None
                        if fused:
                            coefs, recs = plan.round_trip_planes(planes, var_nums=vns)
                        else:
                            coefs, recs = plan.forward_quant_planes(planes, var_nums=vns), None
                        for k in range(2):
                            assert np.array_equal(coefs[k].cpu().numpy(), want_c[k]), (leaf, fused, k)
                            if with_var:
                                assert np.array_equal(vns[k].cpu().numpy().astype(np.float64) / 4096.0, var[k]), (leaf, fused, k)
                            if fused:
                                err = np.abs(recs[k].cpu().numpy().astype(np.float64) - want_r[k]).max()
                                assert err <= 1e-4, (leaf, k, err)
                        if fused:
                            recon = recs
                        n = int(cnt.item())
                        cnt.zero_()
                        if with_cnt:
                            counts[(with_var, fused)] = n
                        else:
                            assert n == 0, leaf
                    plan.set_fallback_counter(None)
            assert counts[(True, False)] == counts[(False, False)] >= dc_ties, (q, ad, counts, dc_ties)
            assert counts[(True, True)] == counts[(False, True)] >= dc_ties, (q, ad, counts, dc_ties)
            # decode8: <adaptive>, <fp32 inverse>, <fp64 inverse> -- the rounded, clamped recon
            gc = [T.from_numpy(c).cuda() for c in want_c]
            gv = [T.from_numpy((v * 4096.0).astype(np.int32)).cuda() for v in var]
            pix = plan.decode_planes(gc, shapes=shapes, var_nums=gv if ad else None)
            for k, (h, w) in enumerate(shapes):
                expect = T.round(recon[k].clamp(0, 255)).to(T.uint8).reshape(h // 8, w // 8, 8, 8)
                assert T.equal(pix[k][0], expect.permute(0, 2, 1, 3).reshape(h, w)), (q, ad, k)
            # idct8_pair, encode_count_kernel, huffman_from_pixels_kernel: the 65-block plane
            rec = plan.inverse(gc[0], var_num=gv[0] if ad else None).cpu().numpy().astype(np.float64)
            assert np.abs(rec - want_r[0]).max() <= 1e-4, (q, ad)
            (ec,), off, sym = plan.encode_planes(planes[:1])
            woff, wsym = O.rle_encode_plane(want_c[0])
            assert np.array_equal(ec.cpu().numpy(), want_c[0]), (q, ad)
            assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), (q, ad)
            assert np.array_equal(_sym32(sym), wsym), (q, ad)
            bits = plan.huffman_bits_planes(planes[:1]).cpu().numpy().view(np.uint32)
            assert np.array_equal(bits, O.huffman_bits_plane(want_c[0])), (q, ad)
