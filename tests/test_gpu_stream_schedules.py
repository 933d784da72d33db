"""Training steps enqueued back to back on the queues the benchmark and every C caller use, against the same steps with the host waiting
after every call.

Every other GPU test creates Context(0) -- torch's legacy default stream -- and reads a result back after nearly every call, so the device has
finished step k before the host enqueues step k + 1.  What a correct step relies on ACROSS queues and ACROSS steps (the fork and the join of the
reconstruction's side stream; recon_join in the pipelined mode; the double-buffered input spectra with ev_end / ev_mid / ev_r2c; the
double-buffered operator sets; the deferred MSE sums riding in the next gradient launch; the context-wide workspaces WS_MID / WS_MID2 / WS_MID3,
each bound to one queue, and the context-wide events, shared by all nets of a context) is invisible to such a test: a missing dependency only
shows when the queues are free to run apart.  Here the same seven-step sequence runs under

  context kinds   torch (Context(0)), own (create_stream = 1: private, non-blocking, highest priority), caller (a caller-owned non-blocking
                  stream), own+partition (own, then aefft_ctx_partition(32): CU-masked queues)
  modes           default, pipelined (set_input_ready(True)), and for one case the development switch NOCHAIN
  host schedules  fenced       aefft_sync + torch.cuda.synchronize() after every library call and every snapshot: the reference
                  back-to-back no host synchronisation between step 1's first enqueue and the final aefft_sync
                  held-back    back-to-back behind device-side delays on the context stream (torch.cuda._sleep): the context stream lags
                               behind the host and behind the side streams for the whole run, so a side-stream kernel that lacks its
                               dependency on the context stream runs early EVERY time.  An event behind the first delay must still be
                               pending when the host has enqueued the last step (asserted in every held-back run: either the delay is too
                               short or a steady-state call synchronises the host, which include/aefft.h promises it does not)

and every snapshot (device copies enqueued on the context stream right behind the call that makes the data valid) and every final weight must
be IDENTICAL: the arithmetic, the launches and the order of the sums depend on neither the queue nor the host, so no comparison here has a
tolerance.  One oracle anchor per case (step 1 of the fenced torch run, teacher-forced from the weights the warm-up step left and the momentum
the rule implies, the bounds of test_gpu_fft_path._step_vs_oracle / test_gpu_spatial_net) ties the shapes to the reference and not only to
each other.

The sequence: step 0 is the warm-up, fenced under every schedule (all first-use allocations happen there); steps 1..6 cycle three frame
batches.  Default mode: ONE staging buffer, refilled by a device copy on the context stream in front of each step_grad.  Pipelined mode: three
resident buffers, complete before step 1 (the mode's contract); a target is staged in both modes (its transform stays on the context
stream).  One reconstruction buffer, NaN-filled on the context stream in front of every step_grad.  step_apply takes mse_d on steps 1 and 4,
None otherwise; last_mse behind step 3 only: the deferred sums cross a step boundary twice without being collected.

Sizing of the delays (measured on an MI355X, this module's back-to-back runs, host time from step 1's first enqueue to the return of the last
call): 0.40 ... 0.84 ms for the one-net cases, 1.03 ... 1.39 ms for two-nets (the largest with the frozen-weight calls in between).  5 x the
largest is 7 ms; FIRST_DELAY_MS = 20 leaves room for a slower host.  STEP_DELAY_MS = 2 in front of every later step_grad and in front of
every step_apply: 20 + 23 * 2 = 66 ms at most per run, under the cap of 200 ms.  (The delay in front of step_apply holds the tail of step k
back until the prefetched input transform of step k + 1, which waits for step k's gradient half only, has run: a transform into the wrong
one of the two input-spectra buffers then overwrites what the per-frame form's tail still reads, every time.  In the operator form the tail
reads second moments, not the input spectra; there only the deferred reconstruction on aux[0] reads them, beside the prefetch on aux[1], and
no delay on the context stream orders two side queues: the schedules catch such a mistake on those nets only through the frozen-weight calls
between the steps, or by chance.)  torch.cuda._sleep counts cycles; their rate is measured once per process (_cycles_per_ms)."""
import functools
import importlib
import time

import numpy as np
import pytest
import torch

import frozen_cases as FC
import np_ref as R
import np_spatial as S
import test_gpu_recon_overlap as RO
import test_gpu_spatial_net as SN
import test_gpu_target as TG
from test_gpu_fft_path import TOL, host, relerr

aefft = importlib.import_module("autoencoder-fft_amd")
pytestmark = pytest.mark.gpu

DEL0, LAST = 0.2, 6                       # steps 1..LAST behind the warm-up step 0
FIRST_DELAY_MS, STEP_DELAY_MS, DELAY_CAP_MS = 20.0, 2.0, 200.0
KINDS = ("torch", "own", "caller", "own+partition")
SCHEDULES = ("fenced", "back-to-back", "held-back")
NETS = {"two-nets": ("64-odd-batch", "96-smooth")}       # a case is one net of its own name, or these on ONE context, stepping in turn
FFT_NETS = ("128-four-pairs", "64-odd-batch", "96-smooth", "64-per-frame", "64-target-u8")
CASE_MODES = {"128-four-pairs": ("default", "pipelined"), "64-odd-batch": ("default", "pipelined", "nochain"), "96-smooth": ("default", "pipelined"),
              "64-per-frame": ("default", "pipelined"), "64-target-u8": ("default", "pipelined"), "spatial": ("default",),
              "two-nets": ("default", "pipelined")}
PARTITION_CASES = ("128-four-pairs", "two-nets")
GRID = [(case, kind, mode) for kind in KINDS for case, modes in CASE_MODES.items() for mode in modes
        if kind != "own+partition" or case in PARTITION_CASES]


@pytest.fixture(scope="module")
def ctx():
    """the torch-stream context behind the `flags` fixture; every run creates (and closes) a context of its own next to it"""
    c = aefft.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------
# the nets: shapes, weights and frames from the modules that own them
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spec(name):
    """shape, weights, three batches of frames (and of targets): computed once, shared by every run, never written to"""
    sp = dict(Nl=None, kw={}, targets=None, spatial=False, form=None, ws=None)
    if name in RO.SHAPES:                      # test_gpu_recon_overlap's nets with its weights and its frames, and two batches more
        N, maps, Nk, B, kw = RO.SHAPES[name]
        ws, x0 = RO._inputs(name)
        rng = np.random.default_rng(1977 + N + len(maps))
        sp.update(D=RO.D, Nx=N, Ny=N, maps=list(maps), Nk=Nk, s=RO.POOL, B=B, kw=kw, ws=ws,
                  frames=[x0] + [np.floor(rng.uniform(0, 256, x0.shape)) for _ in range(2)])
    elif name == "64-per-frame":               # frozen_cases' D = 4 net: the per-frame form
        D, Nx, Ny, maps, Nk, Nl, s, B, *_ = FC.CASES["D4"]
        ws, xs = FC._case("D4")
        sp.update(D=D, Nx=Nx, Ny=Ny, maps=list(maps), Nk=Nk, s=s, B=B, ws=ws, form="per_frame",
                  frames=list(xs) + [np.floor(np.random.default_rng(64).uniform(0, 256, xs[0].shape))])
    elif name == "64-target-u8":               # test_gpu_target's weights and dark targets
        D, N, maps, Nk, B = 3, 64, [4, 3], 5, 2
        rng = np.random.default_rng(6402)
        sp.update(D=D, Nx=N, Ny=N, maps=maps, Nk=Nk, s=2, B=B, ws=TG._weights(rng, D, maps, Nk),
                  frames=[np.floor(rng.uniform(0, 256, (B, D, N, N))) for _ in range(3)],
                  targets=[TG._targets(rng, (B, D, N, N), "dark") for _ in range(3)])
    elif name == "spatial":                    # the smallest two-pair row of test_gpu_spatial_net's step table; weights by its make_net
        D, Nx, Ny, maps, Nk, Nl, s, B, _ = min((r for r in SN.STEP_SHAPES if len(r[3]) == 2), key=lambda r: r[1] * r[2])
        rng = np.random.default_rng(5)
        sp.update(D=D, Nx=Nx, Ny=Ny, maps=list(maps), Nk=Nk, Nl=Nl, s=s, B=B, spatial=True, form="spatial",
                  frames=[SN.frames(rng, B, D, Nx, Ny) for _ in range(3)])
    else:
        raise KeyError(name)
    return sp


def _f64(w):
    return tuple(np.asarray(a).astype(np.float64) for a in w)


# ------------------------------------------------------------------------------------------
# contexts
# ------------------------------------------------------------------------------------------
_partition_refused = []          # the library's error text, once aefft_ctx_partition(32) has failed with AEFFT_EHIP on this machine


def _open(kind):
    if kind == "torch":
        return aefft.Context(0)
    if kind == "caller":
        s = torch.cuda.Stream()                        # non-blocking, the caller's: aefft_ctx_create(create_stream = 0, hip_stream != NULL)
        with torch.cuda.stream(s):
            c = aefft.Context(0)
        c.callers_stream = s                           # lives as long as the context
        assert c.L.aefft_stream(c.h) == s.cuda_stream != 0
        return c
    c = aefft.Context(0, use_torch_stream=False)
    if kind == "own+partition":
        if _partition_refused:
            c.close()
            pytest.skip(f"aefft_ctx_partition(32) fails with AEFFT_EHIP here: {_partition_refused[0]}")
        rc = c.L.aefft_ctx_partition(c.h, 32)
        if rc == aefft.EHIP:
            _partition_refused.append(c.L.aefft_last_error(c.h).decode())
            c.close()
            pytest.skip(f"aefft_ctx_partition(32) fails with AEFFT_EHIP here: {_partition_refused[0]}")
        c.check(rc)
    return c


@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """the rate of torch.cuda._sleep's cycle counter, measured once (a calibration of the delay, not an assertion)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record(); torch.cuda._sleep(2_000_000); b.record()
    torch.cuda.synchronize()
    print(f"torch.cuda._sleep: {2_000_000 / a.elapsed_time(b):.0f} cycles per ms")
    return 2_000_000 / a.elapsed_time(b)


def _delay(ms):
    """plain compute on torch's current stream for about `ms`"""
    torch.cuda._sleep(int(ms * _cycles_per_ms()))


# ------------------------------------------------------------------------------------------
# one net of a run
# ------------------------------------------------------------------------------------------
class _Lane:
    """a net with every buffer its sequence touches -- inputs, staging, reconstruction, one snapshot buffer per step and item -- allocated and
    filled before the sequence starts"""

    def __init__(self, ctx, name, ready, interleave, nets):
        sp = self.sp = _spec(name)
        self.ctx, self.name, self.ready, self.interleave = ctx, name, ready, interleave
        D, Nx, Ny, B = sp["D"], sp["Nx"], sp["Ny"], sp["B"]
        if sp["spatial"]:
            net = SN.make_net(ctx, D, Nx, Ny, sp["maps"], sp["Nk"], sp["Nl"], sp["s"], B, seed=3)
            nets.append(net)
        else:
            net = aefft.Net(ctx, D, Nx, Ny, sp["maps"], sp["Nk"], sp["s"], batch=B, Nl=sp["Nl"], **sp["kw"])
            nets.append(net)
            for l, w in enumerate(sp["ws"]):
                net.set_pair(l, *w)
        self.net, self.L = net, len(sp["maps"])
        self.form = net.step_form()
        if ready:
            net.set_input_ready(True)
        dev = f"cuda:{ctx.device}"
        if sp["targets"] is None:
            self.src, self.tsrc, self.tstage = [ctx.dev(x) for x in sp["frames"]], None, None
        else:                                  # frames as 8-bit pixels, targets as float
            self.src = [torch.as_tensor(x.astype(np.uint8), device=dev) for x in sp["frames"]]
            self.tsrc = [ctx.dev(t) for t in sp["targets"]]
            self.tstage = torch.empty_like(self.tsrc[0])
        self.stage = None if ready else torch.empty_like(self.src[0])
        self.recon, self.mse = ctx.empty(B, D, Nx, Ny), ctx.empty(self.L)
        nan = lambda like: torch.full_like(like, float("nan"))
        self.buf = {}
        for k in range(LAST + 1):
            self.buf[f"{k}.grads"], self.buf[f"{k}.prev"] = nan(net.grad_buffer()), nan(net.mse_prev_global())
            self.buf[f"{k}.recon"] = nan(self.recon)
            if k in (1, 4):
                self.buf[f"{k}.mse"] = nan(self.mse)
            if k == 3:
                self.buf[f"{k}.last_mse"] = nan(self.mse)
            if interleave and k in (0, 2, 4):
                self.buf[f"{k}.infer"], self.buf[f"{k}.score_recon"] = nan(self.recon), nan(self.recon)
                self.buf[f"{k}.score"] = nan(ctx.empty(B))
        if interleave:
            self.other = [ctx.dev(x) for x in FC.other_frames((B, D, Nx, Ny))]
        self.out = {}
        self.w0 = [net.get_pair(l) for l in range(self.L)]

    def take(self, label, src, fence):
        """a device copy on the context stream (torch's current one), right behind the call that made `src` valid"""
        self.buf[label].copy_(src)
        fence()
        self.out[label] = self.buf[label]

    def step(self, k, fence, delay):
        net, i = self.net, k % 3
        self.recon.fill_(float("nan")); fence()
        x = self.src[i]
        if not self.ready:                     # the library must have consumed the previous contents in stream order
            self.stage.copy_(x); fence()
            x = self.stage
        if self.tsrc is not None:
            self.tstage.copy_(self.tsrc[i]); fence()
        delay()
        if self.tsrc is not None:
            net.step_grad_target(x, self.tstage, self.recon)
        else:
            net.step_grad(x, self.recon)
        fence()
        self.take(f"{k}.grads", net.grad_buffer(), fence)
        self.take(f"{k}.prev", net.mse_prev_global(), fence)
        if not self.ready:
            self.take(f"{k}.recon", self.recon, fence)
        if self.sp["spatial"] and k in (0, 1):
            for j, t in enumerate(net.get_layers()):           # (copies on the context stream into a buffer of their own)
                self.out[f"{k}.layer{j}"] = t
            fence()
        delay()                                # (between the gradient half and the tail: what the side queues may do early, they now do)
        net.step_apply(DEL0, 0, 0, 1.0, self.mse if k in (1, 4) else None); fence()
        if self.ready:                         # the deferred reconstruction is complete behind step_apply
            self.take(f"{k}.recon", self.recon, fence)
        if k in (1, 4):
            self.take(f"{k}.mse", self.mse, fence)
        if k == 3:
            net.last_mse(self.buf["3.last_mse"]); fence()
            self.out["3.last_mse"] = self.buf["3.last_mse"]
        if self.interleave and k in (0, 2, 4):                 # frozen-weight calls on unrelated frames, the deferred sums outstanding
            net.infer(self.other[0], self.buf[f"{k}.infer"]); fence()
            net.score(self.other[1], self.buf[f"{k}.score"], self.buf[f"{k}.score_recon"]); fence()
            for what in ("infer", "score", "score_recon"):
                self.out[f"{k}.{what}"] = self.buf[f"{k}.{what}"]
        if self.interleave and k in (0, 5):
            self.out[f"{k}.layer2"] = net.get_layer(2); fence()

    def finish(self):
        net, out = self.net, {k: host(v).copy() for k, v in self.out.items()}
        for l in range(self.L):
            for nme, a in zip("cbfp", net.get_pair(l)):
                out[f"final.{nme}{l}"] = np.asarray(a).copy()
        if self.sp["spatial"]:
            for j, t in enumerate(net.get_layers()):
                out[f"final.layer{j}"] = host(t).copy()
        return out


# ------------------------------------------------------------------------------------------
# one run
# ------------------------------------------------------------------------------------------
_runs = {}


def _run(kind, case, mode, schedule, interleave=False):
    """the sequence of `case` on a fresh context of `kind`: computed once per key and left unchanged.  -> {"lanes": {net name: {label: array}},
    "w0", "w1": {net name: weights before step 0 / before step 1}, "form", "dims", "host_ms", "ahead"}"""
    key = (kind, case, mode, schedule, interleave)
    if key in _runs:
        return _runs[key]
    ctx, nets = _open(kind), []
    try:
        ctx.set_flags(*(["NOCHAIN"] if mode == "nochain" else []))
        res = _sequence(ctx, NETS.get(case, (case,)), nets, mode == "pipelined", schedule, interleave)
    finally:
        while nets:                            # every net before its context
            nets.pop().close()
        ctx.set_flags()
        ctx.close()
    for name, out in res["lanes"].items():
        assert all(np.isfinite(a).all() for a in out.values()), (key, name, [k for k, a in out.items() if not np.isfinite(a).all()])
        last = len(_spec(name)["maps"]) - 1
        assert np.abs(out[f"final.c{last}"] - res["w0"][name][last][0]).max() > 1e-4, "the update was not applied"
    if schedule == "held-back":
        assert res["ahead"], (f"{key}: the event behind the first delay ({FIRST_DELAY_MS} ms) had completed when the host had enqueued the last step "
                              f"({res['host_ms']:.2f} ms of host time): the delay is too short, or a steady-state call synchronises the host")
    print(f"{key}: host time of steps 1..{LAST} {res['host_ms']:.2f} ms, forms {res['form']}")
    _runs[key] = res
    return res


def _sequence(ctx, names, nets, ready, schedule, interleave):
    lanes = [_Lane(ctx, name, ready, interleave, nets) for name in names]
    ctx.sync(); torch.cuda.synchronize()       # inputs uploaded, weights set, buffers filled

    def fenced():
        ctx.sync(); torch.cuda.synchronize()

    free = lambda: None
    held = schedule == "held-back"
    assert FIRST_DELAY_MS + STEP_DELAY_MS * (2 * LAST * len(lanes) - 1) <= DELAY_CAP_MS
    w1, ahead, event = {}, None, None
    with torch.cuda.stream(ctx.torch_stream()):                # everything the test itself enqueues goes on the context stream
        if held:
            _cycles_per_ms()
        for ln in lanes:
            ln.step(0, fenced, free)                           # the warm-up: fenced under every schedule
        for ln in lanes:
            w1[ln.name] = [ln.net.get_pair(l) for l in range(ln.L)]
        fenced()
        fence = fenced if schedule == "fenced" else free
        if held:
            _delay(FIRST_DELAY_MS)
            event = torch.cuda.Event()
            event.record()
        t0 = time.perf_counter()
        skip = [held]                          # step 1's step_grad stands behind the first delay

        def short():
            if held and not skip.pop():
                _delay(STEP_DELAY_MS)
            skip.append(False)

        for k in range(1, LAST + 1):
            for ln in lanes:
                ln.step(k, fence, short)
        host_ms = 1e3 * (time.perf_counter() - t0)
        if held:
            ahead = not event.query()          # the host has returned from the last step_apply (and what the sequence puts behind it)
        ctx.sync()
        torch.cuda.synchronize()
        out = {ln.name: ln.finish() for ln in lanes}
    return dict(lanes=out, w0={ln.name: ln.w0 for ln in lanes}, w1=w1, form={ln.name: ln.form for ln in lanes},
                dims={ln.name: ln.net.dims for ln in lanes}, host_ms=host_ms, ahead=ahead)


def _same(a, b, what):
    """two label -> array tables bit for bit (by label: the pipelined mode takes the reconstruction behind step_apply)"""
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


def _same_run(a, b, what):
    assert list(a["lanes"]) == list(b["lanes"])
    for name in a["lanes"]:
        _same(a["lanes"][name], b["lanes"][name], (what, name))


# ------------------------------------------------------------------------------------------
# the tests
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind,mode", GRID)
def test_host_schedule_changes_no_bit(ctx, flags, case, kind, mode):
    """back-to-back == fenced and held-back == fenced: every snapshot and every final weight; the host-ahead condition in the held-back run"""
    want = _run(kind, case, mode, "fenced")
    for name, form in want["form"].items():
        if _spec(name)["form"] is not None:
            assert form == _spec(name)["form"], (name, form)
        if mode == "nochain":
            assert form == "operator", (name, form)
    for schedule in ("back-to-back", "held-back"):
        _same_run(_run(kind, case, mode, schedule), want, schedule)


@pytest.mark.parametrize("case,kind,mode", [g for g in GRID if g[1] != "torch"])
def test_the_stream_is_not_an_input_of_the_arithmetic(ctx, flags, case, kind, mode):
    """fenced(kind) == fenced(torch), the run that the oracle parity tests pin"""
    _same_run(_run(kind, case, mode, "fenced"), _run("torch", case, mode, "fenced"), kind)


@pytest.mark.parametrize("case,kind", [(c, k) for c, k, m in GRID if m == "pipelined"])
def test_pipelined_fenced_run_gives_the_default_one_s_bits(ctx, flags, case, kind):
    _same_run(_run(kind, case, "pipelined", "fenced"), _run(kind, case, "default", "fenced"), kind)


@pytest.mark.parametrize("mode", ["default", "pipelined"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_nets_on_one_context_step_as_each_alone(ctx, flags, kind, mode):
    """ev_fork, ev_join, recon_join and WS_MID2 / WS_MID3 are the context's, shared by its nets: stepping in turn, under every schedule,
    each net gives what it gives alone on a fresh context of the same kind"""
    for schedule in SCHEDULES:
        both = _run(kind, "two-nets", mode, schedule)
        for name in NETS["two-nets"]:
            alone = _run(kind, name, mode, "fenced")
            _same(both["lanes"][name], alone["lanes"][name], (kind, mode, schedule, name))


@pytest.mark.parametrize("case", list(FFT_NETS) + ["two-nets"])
def test_frozen_weight_calls_between_the_steps(ctx, flags, case):
    """infer and score on unrelated frames behind step_apply of steps 2 and 4, get_layer(2) behind step 5, no synchronisation anywhere: on
    the library's own stream in the pipelined mode, where the calls meet the deferred reconstruction, the prefetched input spectra and
    the outstanding MSE sums.  The schedules agree on every output, and the training is what it is without the calls."""
    want = _run("own", case, "pipelined", "fenced", True)
    for schedule in ("back-to-back", "held-back"):
        _same_run(_run("own", case, "pipelined", schedule, True), want, schedule)
    plain = _run("own", case, "pipelined", "fenced")
    for name, out in plain["lanes"].items():
        mixed = want["lanes"][name]
        assert set(out) < set(mixed)
        _same(out, {k: mixed[k] for k in out}, ("training undisturbed", name))


def test_spatial_net_refuses_the_pipelined_mode(ctx):
    sp, nets = _spec("spatial"), []
    try:
        net = SN.make_net(ctx, sp["D"], sp["Nx"], sp["Ny"], sp["maps"], sp["Nk"], sp["Nl"], sp["s"], sp["B"], seed=3)
        nets.append(net)
        with pytest.raises(aefft.AefftError):
            net.set_input_ready(True)
    finally:
        for n in nets:
            n.close()


@pytest.mark.parametrize("case", FFT_NETS)
def test_step_one_against_the_oracle(ctx, flags, case):
    """step 1 of the fenced torch run, teacher-forced: np_ref.net_step (test_gpu_target.oracle_step for the target) from the weights the
    GPU held behind the warm-up step and the momentum the rule implies (D = w_before - w_after), with the bounds of
    test_gpu_fft_path._step_vs_oracle: reconstruction 1e-4 per frame, gradient segments 5e-5, post-update MSE 1e-5 * max(1, MSE)"""
    run, sp = _run("torch", case, "default", "fenced"), _spec(case)
    out, L = run["lanes"][case], len(sp["maps"])
    w0, w1 = [_f64(w) for w in run["w0"][case]], [_f64(w) for w in run["w1"][case]]
    for a, b in zip(w0, sp["ws"]):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    mom = [(a[0] - b[0], a[2] - b[2], a[1] - b[1], a[3] - b[3]) for a, b in zip(w0, w1)]            # (Dc, Df, Db, Dp) of (c, b, f, p)
    if sp["targets"] is None:
        _, _, mses, recon, grads = R.net_step(sp["frames"][1], w1, mom, sp["s"], DEL0, return_grads=True)
    else:
        ref, recon = TG.oracle_step(sp["frames"][1], sp["targets"][1], w1, mom, sp["s"], dele=0.1 * DEL0)
        mses, grads = [d["mse"] for d in ref], [d["grads"] for d in ref]
    errs = [relerr(out["1.recon"][i], recon[i]) for i in range(sp["B"])]
    print(f"{case}: reconstruction relerr per frame {errs}")
    assert max(errs) < TOL, errs
    for l, segs in enumerate(TG._segments(out["1.grads"], w1)):
        e = [relerr(seg, g.ravel()) for seg, g in zip(segs, grads[l])]
        print(f"{case} pair {l}: gradient relerr {e}, post-update MSE {out['1.mse'][l]:.9g}, oracle {float(mses[l]):.9g}")
        assert max(e) < 5e-5, (l, e)
        assert abs(out["1.mse"][l] - mses[l]) < 1e-5 * max(1, mses[l]), (l, out["1.mse"][l], mses[l])


def test_spatial_step_one_against_the_oracle(ctx, flags):
    """the spatial net's step 1 of the fenced torch run as test_gpu_spatial_net holds a step: packed gradients against np_spatial.gradients
    on the GPU's own layers (5e-5 of the largest entry), the MSE tail and step_apply's MSE against the layers' (1e-4)"""
    run, sp = _run("torch", "spatial", "default", "fenced"), _spec("spatial")
    out, L, B, dims = run["lanes"]["spatial"], len(sp["maps"]), sp["B"], run["dims"]["spatial"]
    assert run["form"]["spatial"] == "spatial"
    w1 = run["w1"]["spatial"]
    segs, tail = SN._grad_segments(out["1.grads"].astype(np.float64), dims)
    for l, g in enumerate(dims):
        xin, o, hin = out[f"1.layer{2 * l + 1}"], out[f"1.layer{4 * L - 1 - 2 * l}"], out[f"1.layer{2 * l + 2}"]
        gs = [S.gradients(xi, oi, hi, w1[l][2]) for xi, oi, hi in zip(xin, o, hin)]
        for nme, ref in zip(("dck", "dfk", "db", "dp"), (sum(t) / B for t in zip(*gs))):
            assert np.abs(segs[l][nme] - ref).max() <= 5e-5 * np.abs(ref).max(), (l, nme)
        ref_mse = ((xin.astype(np.float64) - o) ** 2).sum() / (g["dD"] * g["dM"] * g["Nk"] * g["Nl"] * g["Nx"] * g["Ny"]) / B
        assert abs(tail[l] - ref_mse) <= 1e-4 * ref_mse and abs(out["1.mse"][l] - ref_mse) <= 1e-4 * ref_mse, (l, tail[l], out["1.mse"][l], ref_mse)


def test_partition_and_stream_rules(ctx):
    """aefft_ctx_partition's rules (include/aefft.h) and Context.torch_stream()"""
    lib, ncu = aefft.lib(), torch.cuda.get_device_properties(0).multi_processor_count
    stream = lambda c: lib.aefft_stream(c.h) or 0
    for kind in ("torch", "caller"):           # a context that does not own its stream
        c = _open(kind)
        try:
            assert lib.aefft_ctx_partition(c.h, 32) == aefft.ESTATE
            assert c.torch_stream().cuda_stream == stream(c)
            assert (stream(c) != 0) == (kind == "caller")
        finally:
            c.close()
    c, nets, refused = aefft.Context(0, use_torch_stream=False), [], None
    try:
        for bad in (-1, 7, ncu - 7):
            assert lib.aefft_ctx_partition(c.h, bad) == aefft.EINVAL, bad
        s0 = stream(c)
        assert s0 != 0 and c.torch_stream().cuda_stream == s0
        rc = lib.aefft_ctx_partition(c.h, 32)
        if rc == aefft.EHIP:
            refused = lib.aefft_last_error(c.h).decode()
        else:
            assert rc == aefft.OK, lib.aefft_last_error(c.h).decode()
            s1 = stream(c)
            assert s1 not in (0, s0) and c.torch_stream().cuda_stream == s1
            assert lib.aefft_ctx_partition(c.h, 0) == aefft.OK
            s2 = stream(c)
            assert s2 not in (0, s1) and c.torch_stream().cuda_stream == s2
        nets.append(aefft.Net(c, 3, 64, 64, [4], 5, 2, batch=1))
        assert lib.aefft_ctx_partition(c.h, 32) == aefft.ESTATE       # after the first net
        assert lib.aefft_ctx_partition(c.h, 0) == aefft.ESTATE
    finally:
        for n in nets:
            n.close()
        c.close()
    if refused is not None:
        pytest.skip(f"aefft_ctx_partition(32) fails with AEFFT_EHIP here: {refused} (the other rules hold)")
