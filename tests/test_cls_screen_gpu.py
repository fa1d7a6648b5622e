"""The screened classifier of the greedy generate loop (csrc/kh_cls_screen.h) against the full classifier
(hook KH_CLS_SCREEN=0) on the GPU: identical words, bit-equal logits() behind the run, in graph and fused exec, with a
stop token, behind a prefill; the adversarial vocabularies that force the overflow path; and the cap - no overflow step
on the seeded benchmark image or on the random geometries.

The BASELINE geometries run at their full dim / hidden / heads / vocabulary with two layers (the classifier sees a
residual stream of the same width and statistics; sixteen layers of the same random init add run time, not cases); the
benchmark image itself runs whole."""
import dataclasses

import numpy as np
import pytest
import torch

from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu
PROMPT = [1, 263]
STEPS = 128


def _both(m, fn):
    """fn() under the screened classifier and under KH_CLS_SCREEN=0, with the screen's counters of the first run."""
    try:
        _ffi.debug_set("KH_CLS_SCREEN", None)
        i0 = m.cls_screen_info()
        a = fn()
        i1 = m.cls_screen_info()
        _ffi.debug_set("KH_CLS_SCREEN", "0")
        b = fn()
        i2 = m.cls_screen_info()
    finally:
        _ffi.debug_set("KH_CLS_SCREEN", None)
    assert i2["steps"] == i1["steps"], "KH_CLS_SCREEN=0 still ran screened steps"
    return a, b, {k: i1[k] - i0[k] for k in ("steps", "candidates", "overflow_steps")}


def _same(a, b, what):
    (wa, la), (wb, lb) = a, b
    assert wa == wb, f"{what}: words differ first at {next(i for i, (p, q) in enumerate(zip(wa, wb)) if p != q)}"
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), \
        f"{what}: logits() differ, max |d| {np.abs(la - lb).max()}"


def _run(m, prompt, steps, **kw):
    words, _ = m.generate(prompt, steps, **kw)
    return words, m.logits()


def _check_model(m, label, expect_overflow=False, steps=STEPS):
    info = m.cls_screen_info()
    assert info["on"] == 1 and info["selftest"] == 1, info
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        a, b, d = _both(m, lambda: _run(m, PROMPT, steps))
        log = _ffi.launch_log()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    _same(a, b, f"{label} graph")
    assert any(k.startswith("k_cls_screen<") for k in log) and any(k.startswith("k_sample_screen<") for k in log), log
    assert d["steps"] >= steps, d
    print(f"{label}: {d['steps']} screened steps, {d['candidates'] / max(1, d['steps'] - d['overflow_steps']):.2f} "
          f"candidate rows per step, {d['overflow_steps']} overflow steps")
    if expect_overflow:
        assert d["overflow_steps"] > 0, d
    else:
        assert d["overflow_steps"] == 0, d  # the cap: the overflow path is for the vocabularies built for it
    words = a[0]
    # fused exec, screened, against the graph run
    f, g, _ = _both(m, lambda: _run(m, PROMPT, steps, exec="fused"))
    _same(f, g, f"{label} fused")
    _same(f, a, f"{label} fused vs graph")
    # a stop token hit inside a graph chunk (the first occurrence of the token sampled at step 11)
    stop = [words[11]]
    s1, s0, _ = _both(m, lambda: _run(m, PROMPT, steps, stop=stop))
    _same(s1, s0, f"{label} stop")
    assert len(s1[0]) <= 11
    # behind a prefill (6 fed-only tokens: the B-token path; 20: the GEMM path), first sampled step kept unscreened
    for n in (7, 21):
        prompt = [1] + [int(t) for t in words[:n - 1]]
        p1, p0, dd = _both(m, lambda: _run(m, prompt, n + 40))
        _same(p1, p0, f"{label} prefill {n}")
        assert dd["steps"] > 0
        if not expect_overflow:
            assert dd["overflow_steps"] == 0, dd
    return words


GEOMS = ["llama3.2-1b", "qwen2.5-0.5b", "tinyllama-1.1b"]


@pytest.mark.parametrize("wander", [False, True], ids=["fixed-point", "wander"])
@pytest.mark.parametrize("name", GEOMS)
def test_screened_generate_matches_full_classifier(gpu, name, wander):
    from kuiperllama_amd.model import KuiperModel
    spec = dataclasses.replace(binfmt.PRESETS[name], n_layers=2, seq_len=512)
    img = binfmt.synth_image(spec, seed=77, device=gpu, final_norm_std=1.0 if wander else None)
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec)
    try:
        words = _check_model(m, f"{name} {'wander' if wander else 'fixed-point'}")
        if wander:
            assert len(set(words[2:])) > 8, "the sequence was meant to wander"
    finally:
        m.close()


def test_benchmark_image_never_overflows(gpu):
    """The seeded image bench.py times (Llama-3.2-1B, seed 1234), its prompt, 128 steps."""
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS["llama3.2-1b"]
    img = binfmt.synth_image(spec, seed=1234, device=gpu)
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec)
    try:
        a, b, d = _both(m, lambda: _run(m, PROMPT, STEPS))
        _same(a, b, "benchmark image")
        print(f"benchmark image: {d['candidates'] / d['steps']:.2f} candidate rows per step over {d['steps']} steps")
        assert d["steps"] >= STEPS and d["overflow_steps"] == 0, d  # (+ the first launches of fresh graphs)
        info = m.cls_screen_info()
        assert info["bytes"] == spec.vocab_size * spec.dim * 2 + spec.vocab_size * 4
    finally:
        m.close()


# ---- adversarial vocabularies: dim not a multiple of 256, odd vocabulary, untied classifier --------------------
ADV = binfmt.ModelSpec(448, 1024, 2, 7, 7, 4099, 256, False, binfmt.FAMILY_LLAMA, False, 64,
                       binfmt.ROPE_INTERLEAVED, 10000.0, 1e-5, "adv-448")


def _adv_image(seed=5, wander=True):
    img = binfmt.synth_image(ADV, seed=seed).numpy().copy()
    ents = {e.name: e for e in binfmt.layout(ADV)[0]}

    def view(name):
        e = ents[name]
        return img[e.offset: e.offset + e.nbytes].view(np.float32).reshape(e.shape)
    if wander:  # an untied classifier already wanders; a signed final norm makes it wander more
        view("final_norm")[:] = np.random.default_rng(seed).normal(0, 1, ADV.dim).astype(np.float32)
    return img, view


def _adv_check(img, label, expect_overflow, steps=48):
    from kuiperllama_amd.model import KuiperModel
    m = KuiperModel.from_host_image(np.ascontiguousarray(img), ADV)
    try:
        a, b, d = _both(m, lambda: _run(m, PROMPT, steps))
        _same(a, b, label)
        f, g, _ = _both(m, lambda: _run(m, PROMPT, steps, exec="fused"))
        _same(f, g, label + " fused")
        _same(f, a, label + " fused vs graph")
        print(f"{label}: {d}")
        assert d["steps"] >= steps  # (+ the first launches of fresh graphs)
        assert (d["overflow_steps"] > 0) == expect_overflow, d
        return a[0], d
    finally:
        m.close()


def test_odd_vocabulary_and_dim_not_a_multiple_of_256(gpu):
    img, _ = _adv_image()
    _adv_check(img, "adv plain", expect_overflow=False)


def test_final_norm_all_zeros_gives_token_zero(gpu):
    img, view = _adv_image()
    view("final_norm")[:] = 0
    words, d = _adv_check(img, "adv zero norm", expect_overflow=True)
    assert words[1:] == [0] * (len(words) - 1)  # every logit equal: lowest index (words[0] is the forced prompt token)
    assert d["overflow_steps"] == d["steps"]


def test_two_identical_best_rows_lower_index_wins(gpu):
    img, view = _adv_image()
    base, _ = _adv_check(img, "adv base", expect_overflow=False)
    w = base[1]  # the first sampled token
    lo, hi = (w - 1) % ADV.vocab_size, (w + 1) % ADV.vocab_size
    view("wcls")[lo] = view("wcls")[w]
    view("wcls")[hi] = view("wcls")[w]
    words, _ = _adv_check(img, "adv twins", expect_overflow=False)
    assert words[1] == min(lo, w, hi)


def test_hundreds_of_rows_inside_the_bound_take_the_overflow_path(gpu):
    img, view = _adv_image()
    base, _ = _adv_check(img, "adv base", expect_overflow=False)
    w = base[1]
    W = view("wcls")
    src = W[w].copy()
    for i in range(300):  # copies of the best row with last-bit perturbations
        r = src.copy()
        r[i] = np.nextafter(r[i], np.float32(np.inf) if i % 2 else np.float32(-np.inf))
        W[(w + 1 + 13 * i) % ADV.vocab_size] = r
    _adv_check(img, "adv crowd", expect_overflow=True)


def test_failed_selftest_turns_screening_off(gpu):
    from kuiperllama_amd.model import KuiperModel
    img, _ = _adv_image()
    ref = KuiperModel.from_host_image(np.ascontiguousarray(img), ADV)
    want = _run(ref, PROMPT, 32)
    ref.close()
    try:
        _ffi.debug_set("KH_SELFTEST_FAIL", "screen")
        m = KuiperModel.from_host_image(np.ascontiguousarray(img), ADV)
    finally:
        _ffi.debug_set("KH_SELFTEST_FAIL", None)
    try:
        info = m.cls_screen_info()
        assert info["on"] == 0 and info["selftest"] == -1 and info["bytes"] == 0, info
        _same(_run(m, PROMPT, 32), want, "screening off after a failed self-test")
        assert m.cls_screen_info()["steps"] == 0
    finally:
        m.close()
    m = KuiperModel.from_host_image(np.ascontiguousarray(img), ADV, flags=_ffi.KH_FLAG_NO_CLS_SCREEN)
    try:
        assert m.cls_screen_info()["on"] == 0
        _same(_run(m, PROMPT, 32), want, "KH_FLAG_NO_CLS_SCREEN")
    finally:
        m.close()


def test_entry_points_interleaved_on_one_model_match_an_unscreened_model(gpu):
    """Which step tail is launched, where the classifier reads and writes and whether the logits buffer is behind the
    last step travel as arguments between the entry points: greedy, sampled and greedy generates, time_step, predict,
    the probe and a fused generate, one after the other on ONE model, give the words and logits() of a model created
    without the screen.  The 300-step run crosses position 256, so the screened tail is captured for a second
    attention / wo variant; logits() right behind the probe is k_cls's on the probe's vector."""
    from kuiperllama_amd.model import KuiperModel
    spec = dataclasses.replace(binfmt.PRESETS["tinyllama-1.1b"], n_layers=2, seq_len=512)
    img = binfmt.synth_image(spec, seed=77, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    x = np.random.default_rng(3).normal(0, 1, spec.dim).astype(np.float32)

    def sequence(m, probe):
        out = [("greedy 40",) + _run(m, PROMPT, 40)]
        m.set_sampling(temperature=0.8, top_k=50, seed=7)
        out.append(("sampled 40", m.generate(PROMPT, 40)[0], None))
        m.set_sampling()
        out.append(("greedy 300", m.generate(PROMPT, 300)[0], None))
        m.time_step(5, reps=1)
        out.append(("time_step", [], m.logits()))
        out.append(("predict", [m.predict(out[0][1][3], 3)], m.logits()))
        if probe:
            p = m.cls_screen_probe(x)
            assert p["token"] == p["full_token"] == int(np.argmax(m.logits())), p
        out.append(("fused 40",) + _run(m, PROMPT, 40, exec="fused"))
        return out

    try:
        _ffi.debug_set("KH_CLS_SCREEN", "0")
        plain = KuiperModel.from_device_image(img, spec)
    finally:
        _ffi.debug_set("KH_CLS_SCREEN", None)
    try:
        assert plain.cls_screen_info()["on"] == 0
        want = sequence(plain, probe=False)
        assert plain.cls_screen_info()["steps"] == 0
    finally:
        plain.close()
    m = KuiperModel.from_device_image(img, spec)
    try:
        assert m.cls_screen_info()["on"] == 1
        got = sequence(m, probe=True)
        assert m.cls_screen_info()["steps"] >= 40 + 300 + 40  # (+ the first launches of fresh graphs)
    finally:
        m.close()
    for (what, wa, la), (_, wb, lb) in zip(got, want):
        assert wa == wb, f"{what}: words differ first at {next(i for i, (p, q) in enumerate(zip(wa, wb)) if p != q)}"
        assert (la is None) == (lb is None)
        if la is not None:
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), f"{what}: logits() differ"
    assert len(set(got[2][1][2:])) > 8, "the sequence was meant to wander"
