"""attention_ref (the float64 reference of kx_attention and the checks built on it) validated without a GPU.

1. The reference is the definition: torch's softmax over masked scores, its log-sum-exp, and P |V| of the elementwise bound.
2. A right kernel passes: the float64 restatement of the flash scheme (attention_ref.tiled_attention: 64-key tiles, online
   softmax, P rounded to the P format after exp, l summed from the rounded P) stays inside the probe, parity and lse bounds on
   every shape tests/test_attention_forward_gpu.py launches, and at or below HALF of them.
3. Wrong kernels fail: each of attention_ref.MUTANTS, applied to that restatement, misses the same shared checks on at least one
   of those shapes, for every configuration's bound.
4. The probe inputs see one key: removing or adding a single key moves an element of the row by more than 100 probe bounds."""
import pytest
import torch

import attention_ref as AR

B, H = 2, 3
NAMES = ["bf16", "fp16", "f16c", "fp32"]             # fp32-valu shares fp32's inputs and bounds, bf16-v1 those of bf16
LSE_NAMES = ["bf16", "f16c", "fp32"]
LSE_SHAPES = [(1, 1, True), (65, 65, True), (257, 257, True), (640, 640, True), (64, 321, False), (385, 130, False)]


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """The restatement is hundreds of small float64 matrix products: a thread pool only gets in their way."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _all_shapes():
    return [(tq, tk, c) for c in (True, False) for tq, tk in AR.shapes(c)]


def _worse(a, b):
    return b if b[0] > a[0] else a


def _tiled(kind, name, Tq, Tk, causal, mutant=None):
    dtype, p_fmt, _ = AR.CONFIGS[name]
    q, k, v, R = AR.case(kind, B, H, Tq, Tk, dtype, causal)
    out, lse = AR.tiled_attention(q, k, v, causal, p_fmt, mutant)
    return out, lse, R


def test_the_reference_is_the_definition():
    for Tq, Tk, causal in ((70, 70, True), (5, 131, False)):
        q, k, v = AR.random_qkv(B, H, Tq, Tk, torch.float32, seed=Tq)
        out, lse, P = AR.attention_ref(q, k, v, causal)
        qh, kh, vh = (x.double().permute(0, 2, 1, 3) for x in (q, k, v))
        s = qh @ kh.transpose(-1, -2)
        if causal:
            s = s + torch.triu(torch.full((Tq, Tk), float("-inf"), dtype=torch.float64), 1)
        want = (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Tq, H * 64)
        assert AR.rel_err64(out, want) < 1e-13 and float((lse - torch.logsumexp(s, -1)).abs().max()) < 1e-12
        assert float((P.sum(-1) - 1).abs().max()) < 1e-13 and (not causal or float(P[:, :, 3, 4:].abs().max()) == 0.0)
        # the bound of one element, spelled out
        b = AR.elem_bound(P, v, 2.0 ** -9, 1e-7)
        want_b = 2 * 2.0 ** -9 * sum(float(P[1, 2, 4, j]) * abs(float(v[1, j, 2, 9])) for j in range(Tk)) + 1e-7
        assert abs(float(b[1, 4, 2 * 64 + 9]) - want_b) < 1e-15
        R = AR.Reference(q, k, v, causal)
        # the binade term (attention_ref's docstring) is the P term once more: 4 u_p (P |V|) in all
        assert torch.equal(R.parity_bound("bf16"), AR.elem_bound(P, v, 2.0 ** -8, 2e-5 * R.rms))
        assert torch.equal(R.parity_bound("fp32"), AR.elem_bound(P, v, 0.0, 2e-5 * R.rms))
        assert torch.equal(R.parity_bound("fp16"), AR.elem_bound(P, v, 2.0 ** -11, 2e-5 * R.rms + Tk * 2.0 ** -25 * R.vmax))
        assert torch.equal(R.parity_bound("f16c"), AR.elem_bound(P, v, 0.0, 3e-6 * max(1.0, R.omax)))


def test_the_probe_rows_are_exact_means_and_see_every_key():
    """Probe inputs: the reference row is the exact mean of the value rows the query sees, and one key more or less moves some
    element by more than 100 probe bounds (so a probe launch inside its bound read exactly the right keys)."""
    for T, row, key in ((2, 1, 0), (65, 64, 63), (129, 128, 0), (257, 200, 64), (640, 639, 320), (1025, 1024, 1023), (1025, 511, 7)):
        q, k, v, R = AR.case("probe", B, H, T, T, torch.float32, True)
        vis = v[:, : row + 1].double()
        mean = vis.mean(1).reshape(B, H * 64)
        assert float((R.out[:, row] - mean).abs().max()) < 1e-14
        bound = 2.0 ** -21 * R.out[:, row].abs() + 1e-30
        keep = [j for j in range(row + 1) if j != key]
        removed = v[:, keep].double().mean(1).reshape(B, H * 64)
        added = torch.cat([vis, v[:, key: key + 1].double()], 1).mean(1).reshape(B, H * 64)
        for wrong in (removed, added):
            worst = ((wrong - R.out[:, row]).abs() / bound).reshape(B * H, 64).max(1).values     # per (b, h) row
            assert float(worst.min()) > 100, (T, row, key, float(worst.min()))


def _restatement_ratios(name, family):
    """[(error / bound, shape)] of the unmutated restatement through the shared ratio of a test family, every shape of it."""
    dtype, p_fmt, _ = AR.CONFIGS[name]
    got = []
    if family == "probe":
        for what in _all_shapes():
            out, _, R = _tiled("probe", name, *what)
            got.append((AR.probe_ratio(out, R), what))
    elif family == "parity":
        for what in _all_shapes():
            out, _, R = _tiled("random", name, *what)
            got.append((AR.parity_ratio(name, out, R), what))
        for i in range(len(AR.SPIKES)):
            q, k, v, R, _ = AR.spike_case(dtype, i)
            out, _ = AR.tiled_attention(q, k, v, AR.SPIKES[i][2], p_fmt)
            got.append((AR.parity_ratio(name, out, R), ("spike", i)))
    else:
        for what in LSE_SHAPES:
            _, lse, R = _tiled("random", name, *what)
            got.append((AR.lse_ratio(name, lse, R), what))
    return got


FAMILIES = [(n, f) for n in NAMES for f in ("probe", "parity", "lse") if (n, f) != ("fp16", "lse")]     # (fp16 writes no lse)


@pytest.mark.parametrize("name,family", FAMILIES)
def test_the_restatement_stays_inside_every_bound(name, family):
    """A right kernel passes every shared check on every shape."""
    AR.verdict(_restatement_ratios(name, family), f"restatement, {name} {family}")


@pytest.mark.parametrize("name,family", FAMILIES)
def test_the_restatement_stays_under_half_of_every_bound(name, family):
    """Condition: error / bound <= 0.5 for the unmutated restatement on every shape.
    Worst ratios: probe 0 (the float64 restatement of the probe is exact); parity and lse of f16c and fp32 1e-9 (no P rounding in
    float64); lse bf16 0.34 (T = 257); parity bf16 0.38 (the spike at (300, 130); 0.37 at causal T = 511), fp16 0.34 (causal T = 31).
    The parity bound carries the binade term for this condition (attention_ref's docstring): with 2 u_p (P |V|) alone — ONE
    relative rounding of a P at the bottom of its binade — bf16 sat above 0.5 on 25 of the 31 shapes and at four of the five
    spikes (0.54 .. 0.75) and fp16 on 19 of the 31 shapes (0.50 .. 0.63): rows that lean on a few keys (score std 2.8 here) do
    not average one rounding down.  The mutants below all fail against the bound with the term."""
    AR.verdict(_restatement_ratios(name, family), f"restatement, {name} {family}, half", limit=0.5)


@pytest.mark.parametrize("mutant", AR.MUTANTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_misses_the_parity_bound(name, mutant):
    for Tq, Tk, causal in _all_shapes():
        out, _, R = _tiled("random", name, Tq, Tk, causal, mutant)
        if AR.parity_ratio(name, out, R) > 1.0:
            with pytest.raises(AssertionError):
                AR.verdict([(AR.parity_ratio(name, out, R), (Tq, Tk, causal))], f"{mutant}, {name}")
            return
    pytest.fail(f"{mutant} passes the {name} parity check on every shape")


@pytest.mark.parametrize("mutant", [m for m in AR.MUTANTS if m != "no_rescale"])
def test_every_mutant_but_the_rescale_misses_the_probe_bound(mutant):
    """(q = 0: the maximum never moves, so the probe cannot see a missing rescale; parity and the spikes do.)"""
    out, _, R = _tiled("probe", "fp32", 640, 640, True, "no_rescale")
    assert AR.probe_ratio(out, R) <= 0.5
    for Tq, Tk, causal in _all_shapes():
        out, _, R = _tiled("probe", "bf16", Tq, Tk, causal, mutant)
        if AR.probe_ratio(out, R) > 1.0:
            return
    pytest.fail(f"{mutant} passes the probe check on every shape")


@pytest.mark.parametrize("mutant", AR.MUTANTS)
@pytest.mark.parametrize("name", LSE_NAMES)
def test_every_mutant_misses_the_lse_bound(name, mutant):
    for Tq, Tk, causal in LSE_SHAPES:
        _, lse, R = _tiled("random", name, Tq, Tk, causal, mutant)
        if AR.lse_ratio(name, lse, R) > 1.0:
            return
    pytest.fail(f"{mutant} passes the {name} lse check on every shape")


@pytest.mark.parametrize("name", NAMES)
def test_the_spikes_hold_half_of_a_row_and_catch_a_missed_rescale(name):
    """Every planted key holds 0.3 .. 0.7 of its row; a scheme that does not rescale, or restarts the maximum, or loses the spike's
    key fails the parity check at EVERY spike (the spike sits behind at least one earlier tile, or is the key the row leans on)."""
    dtype, p_fmt, _ = AR.CONFIGS[name]
    for i, (Tq, Tk, causal, query, key) in enumerate(AR.SPIKES):
        q, k, v, R, w = AR.spike_case(dtype, i)
        assert all(0.3 <= x <= 0.7 for x in w), (i, w)
        for mutant in ("no_rescale", "max_reset"):
            if key >= 64:                                                    # (key 5 sits in the first tile: nothing to rescale yet)
                out, _ = AR.tiled_attention(q, k, v, causal, p_fmt, mutant)
                assert AR.parity_ratio(name, out, R) > 100, (i, mutant)
        k2, v2 = k.clone(), v.clone()
        k2[:, key], v2[:, key] = k[:, key - 1], v[:, key - 1]                # the spike's key lost (its neighbour read in its place)
        out, _ = AR.tiled_attention(q, k2, v2, causal, p_fmt)
        assert AR.parity_ratio(name, out, R) > 100, i
