"""The zonal spectra on the device (csrc/wx_spectrum.h through the raw C ABI and through wxengine/spectrum.py) against the fixtures
(tests/golden/spectrum_*.npz, the reference's own classes) and the fp64 oracle (tests/spectrum_oracle.py).

The bars are derived, not tuned.  The device sums in fp64 and rounds once, so with a_h the mean |r| of a row, u = 2^-53 and
delta_h = (W + 8) u a_h -- the relative error of an fp64 sum of W products with twiddles good to u, times a_h:
  PSD per bin    |X_k| <= W a_h and its error <= W delta_h, so psd = mult |X|^2 / W^2 is off by at most 2 mult a_h delta_h = 4 a_h delta_h;
                 the bar doubles that and adds the one float32 rounding:   |dev - psd64| <= 2^-23 psd64 + 8 a_h delta_h
                 (about 8e-8 at W = 1440 and a = 250, against PSD values of 2e-7 to 1e5), and over a case
                 max|dev - psd64| <= E_ref = max|psd32 - psd64|: the device is no further from fp64 than the reference's float32 run.
  mean PSD       a weighted mean of the rows' PSD (weights what_h >= 0 that sum to 1): the same 8 a delta with a = max_h a_h, plus
                 H 2^-52 relative for the H-term fp64 sum in an order that differs from the oracle's; relative to the oracle value.
  mean amplitude |X| is off by at most W delta_h, the mean by at most (sum_h w_h / H) W delta; doubled like the PSD's, plus H 2^-52.
  scores         relative error against the fp64 oracle <= R_ref, the largest relative float32 error of the reference's own two losses
                 over s0 - s4, computed here from the fixtures: a condition the reference itself meets by construction.
Everything else is bit for bit: independence of the plane count, the position and the split of a call, strided views, psd with and
without a second field, compare(x, x), and weights of one against no weights.  Every output lies between guard bands."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import spectrum_cases as SC  # noqa: E402
import spectrum_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GUARD, FILL = 96, -7777.25
U = 2.0 ** -53
CASES = list(SC.SPECTRUM_CASES)


@pytest.fixture(scope="module")
def lib():
    from wxengine.engine import load_library
    return load_library()


@pytest.fixture(scope="module")
def goldens():
    return {name: SC.load_golden(name, GOLD) for name in CASES}


@pytest.fixture(scope="module")
def inputs():
    """Per case the fields on the host and on the device, the weights and the fp64 oracle's quantities: computed once, never changed."""
    out = {}
    for name in CASES:
        pred, target = SC.fields(name)
        w, k = SC.weights(name), SC.SPECTRUM_CASES[name]["k_init"]
        out[name] = dict(pred=pred, target=target, w=w, k_init=k, dpred=torch.from_numpy(pred).cuda(), dtarget=torch.from_numpy(target).cuda(),
                         mean_psd=(SO.mean_psd(pred, w), SO.mean_psd(target, w)), mean_amp=(SO.mean_amp(pred, w), SO.mean_amp(target, w)),
                         scores=SO.scores(pred, target, k, w))
    return out


def guarded(shape, dtype=torch.float32):
    """-> (buffer, view of `shape` between two guard bands of FILL)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), FILL, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_ok(buf):
    return bool((buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all())


class Raw:
    """One handle of the raw C ABI."""

    def __init__(self, lib, H, W, w=None):
        self.lib, self.H, self.W, self.Wh = lib, H, W, W // 2 + 1
        self.h = C.c_void_p()
        lw = None if w is None else np.ascontiguousarray(w, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
        assert lib.wx_spectrum_create(H, W, lw, 0, C.byref(self.h)) == 0, lib.wx_last_error()

    def close(self):
        assert self.lib.wx_spectrum_destroy(self.h) == 0

    def apply(self, P, a, b=None, k_init=0, a_stride=None, b_stride=None, **outs):
        """outs: psd_a, psd_b, mean_psd_a, mean_psd_b, mean_amp_a, mean_amp_b, scores -- device tensors or absent.  -> status"""
        hw = self.H * self.W
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
        order = ("psd_a", "psd_b", "mean_psd_a", "mean_psd_b", "mean_amp_a", "mean_amp_b", "scores")
        assert set(outs) <= set(order)
        return self.lib.wx_spectrum_apply(self.h, P, p(a), hw if a_stride is None else a_stride, p(b), hw if b_stride is None else b_stride,
                                          k_init, *[p(outs.get(n)) for n in order], C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def everything(self, a, b, k_init):
        """All seven outputs of a call on contiguous [P, H, W] fields, between guard bands -> dict of host arrays."""
        P = a.shape[0]
        shapes = dict(psd_a=((P, self.H, self.Wh), torch.float32), psd_b=((P, self.H, self.Wh), torch.float32),
                      mean_psd_a=((P, self.Wh), torch.float64), mean_psd_b=((P, self.Wh), torch.float64),
                      mean_amp_a=((P, self.Wh), torch.float64), mean_amp_b=((P, self.Wh), torch.float64), scores=((P, 2), torch.float64))
        bufs = {n: guarded(s, d) for n, (s, d) in shapes.items()}
        keep_a, keep_b = a.clone(), b.clone()
        assert self.apply(P, a, b, k_init, **{n: v for n, (_, v) in bufs.items()}) == 0, self.lib.wx_last_error()
        torch.cuda.synchronize()
        assert all(guards_ok(buf) for buf, _ in bufs.values()) and torch.equal(a, keep_a) and torch.equal(b, keep_b)
        return {n: v.cpu().numpy() for n, (_, v) in bufs.items()}


@pytest.fixture(scope="module")
def device_results(lib, inputs):
    """One call per case with every output: shared by the accuracy tests."""
    out = {}
    for name, c in inputs.items():
        P, H, W = c["pred"].shape
        r = Raw(lib, H, W, c["w"])
        out[name] = r.everything(c["dpred"], c["dtarget"], c["k_init"])
        r.close()
    return out


def row_scale(x):
    """a_h: [P, H] mean |r| per row, float64."""
    return np.abs(x.astype(np.float64)).mean(axis=-1)


@pytest.mark.parametrize("name", CASES)
def test_psd_is_within_both_bars(goldens, inputs, device_results, name):
    g, c = goldens[name], inputs[name]
    W = c["pred"].shape[-1]
    got = device_results[name]["psd_a"].astype(np.float64)
    err = np.abs(got - g["psd64"])
    a = row_scale(c["pred"])[..., None]
    bar = 2.0 ** -23 * g["psd64"] + 8.0 * a * ((W + 8) * U * a)
    print(f"spectrum {name}: max|dev - psd64| {err.max():.3e} = {err.max() / float(g['E_ref']):.2e} E_ref; worst bin at {(err / bar).max():.3f} of its bar "
          f"(accumulation term {(8.0 * a * ((W + 8) * U * a)).max():.2e})")
    assert np.isfinite(got).all()
    assert err.max() <= float(g["E_ref"])
    assert (err <= bar).all(), f"{name}: bin {np.unravel_index(np.argmax(err / bar), err.shape)} is {(err / bar).max():.3f} of its bar"
    # the second field's PSD obeys the same bar against the oracle
    tgt = device_results[name]["psd_b"].astype(np.float64)
    want = SO.psd(c["target"])
    at = row_scale(c["target"])[..., None]
    assert (np.abs(tgt - want) <= 2.0 ** -23 * want + 8.0 * at * ((W + 8) * U * at)).all()


@pytest.mark.parametrize("name", CASES)
def test_mean_spectra_are_within_the_accumulation_bar(inputs, device_results, name):
    c, d = inputs[name], device_results[name]
    P, H, W = c["pred"].shape
    wsum_over_h = float(c["w"].astype(np.float64).sum()) / H
    for i, field in enumerate(("pred", "target")):
        a = row_scale(c[field]).max(axis=-1)[:, None]                      # [P, 1]
        delta = (W + 8) * U * a
        for what, got, want, acc in (("mean_psd", d["mean_psd_" + "ab"[i]], c["mean_psd"][i], 8.0 * a * delta),
                                     ("mean_amp", d["mean_amp_" + "ab"[i]], c["mean_amp"][i], 2.0 * wsum_over_h * W * delta)):
            rel = np.abs(got - want) / want
            bar = acc / want + H * 2.0 ** -52
            print(f"spectrum {name} {what} {field}: max relative error {rel.max():.3e}, worst bin at {(rel / bar).max():.3f} of its bar")
            assert (rel <= bar).all(), (name, what, field)


def test_scores_and_losses_are_within_the_reference_s_own_error(lib, goldens, inputs, device_results):
    from wxengine.spectrum import ZonalSpectrum
    r_ref = SC.r_ref(goldens)
    assert 1e-7 < r_ref < 1e-3
    for name in CASES:
        g, c = goldens[name], inputs[name]
        got = device_results[name]["scores"]
        rel = np.abs(got - c["scores"]) / np.abs(c["scores"])
        rel_g = np.abs(got - g["scores64"]) / np.abs(g["scores64"])
        loss_rel = np.abs(got.mean(axis=0) - g["loss64"]) / np.abs(g["loss64"])
        vs32 = np.abs(got.mean(axis=0) - g["loss32"].astype(np.float64)) / np.abs(g["loss64"])
        print(f"spectrum {name}: scores relative error {rel.max():.3e} (fixture {rel_g.max():.3e}), losses {loss_rel.max():.3e}; "
              f"from the reference's float32 losses {vs32.max():.3e}; R_ref {r_ref:.3e}")
        assert rel.max() <= r_ref and rel_g.max() <= r_ref and loss_rel.max() <= r_ref
        assert vs32.max() <= 2 * r_ref
        # the class gives the raw call's bits, the reference's two scalars and the blurring curve
        P, H, W = c["pred"].shape
        res = ZonalSpectrum(H, W, lat_weights=c["w"]).compare(c["dpred"], c["dtarget"], wavenum_init=c["k_init"])
        assert np.array_equal(res.psd_score, got[:, 0]) and np.array_equal(res.amp_score, got[:, 1])
        assert res.psd_loss == got[:, 0].mean() and res.spectral_loss == got[:, 1].mean()
        d = device_results[name]
        assert np.array_equal(res.mean_psd_pred, d["mean_psd_a"]) and np.array_equal(res.mean_psd_target, d["mean_psd_b"])
        assert np.array_equal(res.mean_amp_pred, d["mean_amp_a"]) and np.array_equal(res.mean_amp_target, d["mean_amp_b"])
        assert np.array_equal(res.ratio, d["mean_psd_a"] / d["mean_psd_b"]) and res.ratio.shape == (P, W // 2 + 1)


def test_a_plane_does_not_depend_on_the_call_around_it(lib, inputs, device_results):
    c, full = inputs["s2"], device_results["s2"]
    P, H, W = c["pred"].shape
    r = Raw(lib, H, W, c["w"])
    # one plane per call, last plane first: a smaller scratch than the full call's, another position, another plane count
    for p in reversed(range(P)):
        one = r.everything(c["dpred"][p:p + 1], c["dtarget"][p:p + 1], c["k_init"])
        for n, v in one.items():
            assert np.array_equal(v[0], full[n][p]), (p, n)
    # a split 2 + 3 and the planes in another order inside the batch
    perm = [3, 0, 4, 2, 1]
    shuffled = r.everything(c["dpred"][perm].contiguous(), c["dtarget"][perm].contiguous(), c["k_init"])
    head = r.everything(c["dpred"][:2], c["dtarget"][:2], c["k_init"])
    tail = r.everything(c["dpred"][2:], c["dtarget"][2:], c["k_init"])
    for n, v in full.items():
        assert np.array_equal(shuffled[n], v[perm]), n
        assert np.array_equal(np.concatenate([head[n], tail[n]]), v), n
    # planes at a stride: every second plane of a wider buffer, the second field one float into its own
    wide = torch.full((2 * P, H, W), 3.0, device="cuda")
    wide[::2] = c["dpred"]
    off = torch.full((P * H * W + 1,), 5.0, device="cuda")
    off[1:] = c["dtarget"].reshape(-1)
    bufs = {n: guarded(full[n].shape, torch.float32 if n.startswith("psd") else torch.float64) for n in full}
    assert r.apply(P, wide, off[1:], c["k_init"], a_stride=2 * H * W, **{n: v for n, (_, v) in bufs.items()}) == 0, lib.wx_last_error()
    torch.cuda.synchronize()
    for n, (buf, v) in bufs.items():
        assert guards_ok(buf) and np.array_equal(v.cpu().numpy(), full[n]), n
    r.close()


def test_psd_of_a_is_the_same_with_and_without_b(lib, inputs, device_results):
    for name in ("s0", "s3"):
        c, full = inputs[name], device_results[name]
        P, H, W = c["pred"].shape
        r = Raw(lib, H, W, c["w"])
        buf, psd = guarded(full["psd_a"].shape)
        mbuf, mean = guarded(full["mean_psd_a"].shape, torch.float64)
        abuf, amp = guarded(full["mean_amp_a"].shape, torch.float64)
        assert r.apply(P, c["dpred"], psd_a=psd, mean_psd_a=mean, mean_amp_a=amp) == 0, lib.wx_last_error()
        torch.cuda.synchronize()
        assert guards_ok(buf) and guards_ok(mbuf) and guards_ok(abuf)
        assert np.array_equal(psd.cpu().numpy(), full["psd_a"]) and np.array_equal(mean.cpu().numpy(), full["mean_psd_a"])
        assert np.array_equal(amp.cpu().numpy(), full["mean_amp_a"])
        r.close()


def test_a_field_against_itself_scores_zero_and_has_ratio_one(inputs):
    from wxengine.spectrum import ZonalSpectrum
    for name in ("s1", "s3"):
        c = inputs[name]
        P, H, W = c["pred"].shape
        spec = ZonalSpectrum(H, W, lat_weights=c["w"])
        for other in (c["dpred"], c["dpred"].clone()):
            res = spec.compare(c["dpred"], other, wavenum_init=c["k_init"])
            assert np.array_equal(res.psd_score, np.zeros(P)) and np.array_equal(res.amp_score, np.zeros(P))
            assert res.psd_loss == 0.0 and res.spectral_loss == 0.0 and np.array_equal(res.ratio, np.ones((P, W // 2 + 1)))


def test_no_weights_are_weights_of_one(lib, inputs):
    c = inputs["s2"]
    P, H, W = c["pred"].shape
    plain, ones = Raw(lib, H, W), Raw(lib, H, W, np.ones(H, dtype=np.float32))
    a, b = plain.everything(c["dpred"], c["dtarget"], 3), ones.everything(c["dpred"], c["dtarget"], 3)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    # mean_psd without weights is the plain mean over the rows: what = 1 / H
    want = SO.mean_psd(c["pred"])
    amax = row_scale(c["pred"]).max()
    assert (np.abs(a["mean_psd_a"] - want) / want).max() <= 8.0 * amax ** 2 * (W + 8) * U / want.min() + H * 2.0 ** -52
    plain.close()
    ones.close()


def test_the_raw_abi_refuses_before_it_launches(lib, inputs):
    c = inputs["s0"]
    P, H, W = c["pred"].shape
    Wh, hw = W // 2 + 1, H * W
    r = Raw(lib, H, W, c["w"])
    a, b = c["dpred"], c["dtarget"]
    buf, psd = guarded((P, H, Wh))
    sbuf, scores = guarded((P, 2), torch.float64)
    mbuf, mean = guarded((P, Wh), torch.float64)

    def refused(why, status):
        assert status == -1 and why.encode() in lib.wx_last_error(), (why, lib.wx_last_error())

    refused("n_planes must be >= 1", r.apply(0, a, psd_a=psd))
    refused("null pointer", r.apply(P, None, psd_a=psd))
    refused("a scores pointer needs b", r.apply(P, a, scores=scores))
    refused("an output of b needs b", r.apply(P, a, psd_a=psd, mean_psd_b=mean))
    refused("no output requested", r.apply(P, a, b))
    refused("k_init must be in 0 .. W / 2 = 6, got -1", r.apply(P, a, b, -1, scores=scores))
    refused("k_init must be in 0 .. W / 2 = 6, got 7", r.apply(P, a, b, Wh, scores=scores))
    refused("stride is smaller than H * W", r.apply(P, a, b, a_stride=hw - 1, scores=scores))
    refused("beyond 2^44", r.apply(P, a, b, b_stride=1 << 60, scores=scores))
    refused("an output overlaps an input", r.apply(P, a, b, psd_a=a[1:]))
    refused("an output overlaps an input", r.apply(P, a, b, scores=b.view(torch.float64)[2:]))
    refused("two outputs overlap", r.apply(P, a, b, psd_a=psd, psd_b=psd.reshape(-1)[Wh:]))
    torch.cuda.synchronize()
    assert guards_ok(buf) and guards_ok(sbuf) and guards_ok(mbuf)
    assert (psd == FILL).all() and (scores == FILL).all() and torch.equal(a.cpu(), torch.from_numpy(c["pred"]))
    assert lib.wx_spectrum_apply(None, P, None, hw, None, hw, 0, *([None] * 7), None) == -1 and b"null spectrum handle" in lib.wx_last_error()
    r.close()


def test_the_class_takes_any_leading_shape_strided_views_and_named_tensors(inputs, device_results):
    from wxengine.spectrum import ZonalSpectrum
    c, full = inputs["s2"], device_results["s2"]
    P, H, W = c["pred"].shape                                   # 5 planes
    Wh = W // 2 + 1
    spec = ZonalSpectrum(H, W, lat_weights=c["w"])
    psd = spec.psd(c["dpred"])
    assert psd.dtype == torch.float32 and tuple(psd.shape) == (P, H, Wh) and np.array_equal(psd.cpu().numpy(), full["psd_a"])
    assert np.array_equal(spec.psd(c["dpred"][3]).cpu().numpy(), full["psd_a"][3])                  # [H, W]
    x5 = c["dpred"][:4].reshape(1, 2, 2, H, W)
    assert np.array_equal(spec.psd(x5).cpu().numpy(), full["psd_a"][:4].reshape(1, 2, 2, H, Wh))
    mean = spec.mean_spectrum(x5)
    assert mean.dtype == torch.float64 and np.array_equal(mean.cpu().numpy(), full["mean_psd_a"][:4].reshape(1, 2, 2, Wh))
    wide = torch.zeros((1, 9, H, W), device="cuda")
    wide[0, 2:7] = c["dpred"]
    assert np.array_equal(spec.psd(wide[:, 2:7]).cpu().numpy()[0], full["psd_a"])                   # a channel slice, read where it lies
    assert np.array_equal(spec.psd(wide[0, 2:7:2]).cpu().numpy(), full["psd_a"][::2])               # every second plane
    padded = torch.zeros((P, H, W + 3), device="cuda")
    padded[..., :W] = c["dpred"]
    assert np.array_equal(spec.psd(padded[..., :W]).cpu().numpy(), full["psd_a"])                   # rows not contiguous: copied
    # named tensors: {source: {var: [1, L, 1, H, W]}}, keys sorted, a variable of L levels is L planes
    tw = torch.zeros((1, 9, H, W), device="cuda")
    tw[0, 2:7] = c["dtarget"]
    pred = {"era5": {"v": wide[:, 2:5].unsqueeze(2), "t": wide[:, 5:7].unsqueeze(2)}}
    target = {"t": tw[:, 5:7].unsqueeze(2), "v": tw[:, 2:5].unsqueeze(2)}
    res = spec.compare(pred, target, wavenum_init=c["k_init"])
    assert list(res) == ["t", "v"]
    assert res["v"].psd_score.shape == (1, 3, 1) and np.array_equal(res["v"].psd_score.reshape(-1), full["scores"][:3, 0])
    assert np.array_equal(res["t"].amp_score.reshape(-1), full["scores"][3:, 1]) and res["t"].mean_psd_pred.shape == (1, 2, 1, Wh)
    assert np.array_equal(res["t"].mean_psd_target.reshape(2, Wh), full["mean_psd_b"][3:])
    assert res["v"].psd_loss == full["scores"][:3, 0].mean()


def test_spectra_of_rollout_equals_per_step_compare_without_a_sync(inputs, monkeypatch):
    from wxengine.rollout import spectra_of_rollout
    from wxengine.spectrum import PendingSpectra, ZonalSpectrum
    c = inputs["s2"]
    P, H, W = c["pred"].shape
    spec = ZonalSpectrum(H, W, lat_weights=c["w"])
    noise = torch.from_numpy(SC.fields("s2")[1] - SC.fields("s2")[0]).cuda()
    out = [c["dpred"].unsqueeze(0).clone(), (c["dpred"] + 2 * noise).unsqueeze(0)]                  # two steps of [1, C, H, W]
    targets = [c["dtarget"].unsqueeze(0).clone(), {"t": c["dtarget"][3:].unsqueeze(0).unsqueeze(2), "v": c["dtarget"][:3].unsqueeze(0).unsqueeze(2)}]
    cmap = {"v": slice(0, 3), "t": {"slice": slice(3, 5)}}
    want = [spec.compare({k: y[:, sl].unsqueeze(2) for k, sl in (("v", slice(0, 3)), ("t", slice(3, 5)))},
                         {k: c["dtarget"][sl].unsqueeze(0).unsqueeze(2) for k, sl in (("v", slice(0, 3)), ("t", slice(3, 5)))}, 3) for y in out]
    torch.cuda.synchronize()

    def no_sync(*_a, **_k):
        raise AssertionError("spectra_of_rollout waited for the device")
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "synchronize", no_sync)
        m.setattr(torch.cuda.Event, "synchronize", no_sync)
        m.setattr(torch.cuda.Stream, "synchronize", no_sync)
        m.setattr(torch.Tensor, "cpu", no_sync)
        m.setattr(torch.Tensor, "item", no_sync)
        pending = spectra_of_rollout(out, targets, spec, cmap, wavenum_init=3)
    assert len(pending) == 2 and all(isinstance(p, PendingSpectra) for p in pending)
    for p, w in zip(pending, want):
        got = p.result()
        assert list(got) == ["t", "v"] and p.done()
        for k in got:
            for part in ("psd_score", "amp_score", "mean_psd_pred", "mean_psd_target", "mean_amp_pred", "mean_amp_target", "ratio"):
                assert np.array_equal(getattr(got[k], part), getattr(w[k], part)), (k, part)
            assert got[k].psd_loss == w[k].psd_loss and got[k].spectral_loss == w[k].spectral_loss
    with pytest.raises(ValueError, match="one entry per step"):
        spectra_of_rollout(out, targets[:1], spec, cmap)
