"""Acceleration limits on the sampled controls, on the host: csrc/control_limits.h compiled with g++ on its own -- the
recurrence the kernel walks -- against the numpy model (tests/control_limits_model.py) bit for bit, and the model's own
property: every limited sequence, and every weighted mean of them as the update forms it, is feasible within
tol = 2^-20 * (M + d).  The GPU tests lean on that property; it has to hold for the model alone, here."""
import os
import struct
import subprocess

import numpy as np
import pytest

import control_limits_model as model

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "control_limits.h")
F = np.float32

# stdin: cases of {int32 T, int32 N, float lo, hi, anchor, accel, dt, u[T], e[N][T]}; stdout per case: d, e'[N][T].
# With an argument: stdin floats, stdout one uint32 per float, control_limit_valid.
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "%s"
int main(int argc, char**) {
  if (argc > 1) {
    float a;
    while (std::fread(&a, 4, 1, stdin) == 1) {
      const uint32_t ok = (uint32_t)mppi::control_limit_valid(a);
      std::fwrite(&ok, 4, 1, stdout);
    }
    return 0;
  }
  int32_t shape[2];
  while (std::fread(shape, 4, 2, stdin) == 2) {
    const int T = shape[0], N = shape[1];
    float head[5];
    if (std::fread(head, 4, 5, stdin) != 5) return 2;
    std::vector<float> u((size_t)T), e((size_t)N * T);
    if (std::fread(u.data(), 4, u.size(), stdin) != u.size()) return 2;
    if (std::fread(e.data(), 4, e.size(), stdin) != e.size()) return 2;
    const float d = mppi::control_limit_step_size(head[3], head[4]);
    for (int n = 0; n < N; ++n) mppi::control_limit_chain(u.data(), 1, e.data() + (size_t)n * T, 1, T, head[0], head[1], head[2], d);
    std::fwrite(&d, 4, 1, stdout);
    std::fwrite(e.data(), 4, e.size(), stdout);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("control_limits")
    src = tmp / "chain.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp / "chain"
    # -O2 with fused multiply-add available to the compiler: nothing in the header may be contracted or reassociated
    flags = ["-O2", "-ffp-contract=fast"] + (["-mfma"] if os.uname().machine in ("x86_64", "AMD64") else [])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", str(exe), str(src)])

    def chains(cases):
        """cases: (u (T,), e (N, T), lo, hi, anchor, accel, dt) -> [(d, e' (N, T))]"""
        blob = b""
        for u, e, lo, hi, anchor, accel, dt in cases:
            blob += struct.pack("<ii", e.shape[1], e.shape[0]) + np.array([lo, hi, anchor, accel, dt], dtype=F).tobytes()
            blob += np.ascontiguousarray(u, dtype=F).tobytes() + np.ascontiguousarray(e, dtype=F).tobytes()
        raw = np.frombuffer(subprocess.run([str(exe)], input=blob, stdout=subprocess.PIPE, check=True).stdout, dtype=F)
        out, at = [], 0
        for u, e, *_ in cases:
            out.append((raw[at], raw[at + 1:at + 1 + e.size].reshape(e.shape)))
            at += 1 + e.size
        assert at == len(raw)
        return out

    def valid(values):
        raw = subprocess.run([str(exe), "valid"], input=np.asarray(values, dtype=F).tobytes(), stdout=subprocess.PIPE, check=True).stdout
        return np.frombuffer(raw, dtype=np.uint32)
    chains.valid = valid
    return chains


def cases():
    """name -> (u (T,), e (N, T), lo, hi, anchor, accel, dt): what the issue lists, 256 chains of 50 steps each."""
    rng = np.random.default_rng(2)
    n, t = 256, 50

    def normal(std, shape=(n, t)):
        return (rng.normal(0, 1, shape) * std).astype(F)
    out = {}
    out["box"] = (rng.uniform(0, 1, t).astype(F), normal(2.0), 0.0, 1.0, 0.5, 100.0, 0.1)
    out["rate"] = (rng.uniform(-1, 1, t).astype(F), normal(1.0), -1.0, 1.0, 0.25, 1.0, 0.1)
    u = (0.5 + 0.01 * np.arange(t)).astype(F)
    out["nothing"] = (u, normal(0.01), -10.0, 10.0, float(u[0]), 100.0, 0.1)
    out["freeze"] = (rng.uniform(0.5, 4, t).astype(F), normal(1.0), 0.5, 4.0, 1.0, 1e-8, 0.1)
    out["denormal"] = (np.zeros(t, dtype=F), normal(1e-40), -1.0, 1.0, 0.0, 1e-38, 0.1)
    u = rng.uniform(-1, 1, t).astype(F)
    e = np.broadcast_to(-u, (n, t)).copy()
    e[n // 2:] = (e[n // 2:].astype(np.float64) * (1 + rng.integers(-3, 4, (n - n // 2, t)) * 2.0 ** -24)).astype(F)
    out["cancel"] = (u, e, -1.0, 1.0, 0.1, 0.5, 0.1)
    out["anchor_above"] = (rng.uniform(0.1, 1, t).astype(F), normal(0.5), 0.1, 1.0, 5.0, 2.0, 0.1)
    out["anchor_below"] = (rng.uniform(0.1, 1, t).astype(F), normal(0.5), 0.1, 1.0, -3.0, 2.0, 0.1)
    out["away_from_zero"] = (rng.uniform(0.2, 1.5, t).astype(F), normal(0.7), 0.2, 1.5, 0.9, 3.0, 0.05)
    out["one_step"] = (rng.uniform(-1, 1, 1).astype(F), normal(1.0, (n, 1)), -1.0, 1.0, 0.3, 1.0, 0.1)
    out["no_limit"] = (rng.uniform(-1, 1, t).astype(F), normal(1.0), -1.0, 1.0, 0.3, np.inf, 0.1)
    return out


def test_the_header_agrees_with_the_model_bit_for_bit(header):
    named = cases()
    got = header(list(named.values()))
    steps = 0
    for (name, (u, e, lo, hi, anchor, accel, dt)), (d, out) in zip(named.items(), got):
        want_d = model.step_size(accel, dt)[0]
        assert F(d).view(np.uint32) == want_d.view(np.uint32), name
        want, path = model.chain(e, u, lo, hi, anchor, want_d)
        bad = out.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%s: %d of %d steps differ, first at %s" % (name, bad.sum(), bad.size, np.argwhere(bad)[:1])
        steps += e.size
        # the cases reach what they are there for
        c = model.clip(np.add(u[None, :], e, dtype=F), lo, hi)
        raw = np.add(u[None, :], e, dtype=F)
        if name == "box":
            assert ((raw < lo) | (raw > hi)).mean() > 0.3 and (path == c).mean() > 0.9
        if name == "rate":
            before = np.concatenate([np.full((len(e), 1), model.clip(F(anchor), lo, hi)), path[:, :-1]], axis=1)
            assert ((path != c) & (path > before)).sum() > 1000 and ((path != c) & (path < before)).sum() > 1000
        if name == "nothing":
            assert np.abs(out - e).max() < 1e-6 and (path == raw).all()  # (e' = fl(fl(u + e) - u): e up to rounding)
        if name == "freeze":
            assert (path == F(1.0)).all() and (c != F(1.0)).all() and want_d < 2.0 ** -25
        if name == "denormal":
            assert ((np.abs(e) > 0) & (np.abs(e) < 2.0 ** -126)).mean() > 0.9 and 0 < want_d < 2.0 ** -126 and (path != 0).any()
        if name == "cancel":
            assert (raw[:len(e) // 2] == 0).all() and (raw[len(e) // 2:] != 0).any()
        if name.startswith("anchor"):
            first = model.clip(F(anchor), lo, hi)
            assert first in (F(lo), F(hi)) and (np.abs(path[:, 0].astype(np.float64) - float(first)) <= float(want_d) + 2.0 ** -22).all()
        if name == "one_step":
            assert out.shape == (256, 1) and (out != e).any()
        if name == "no_limit":
            assert np.isinf(want_d) and (out.view(np.uint32) == e.view(np.uint32)).all(), "a component at inf returns its input's bits"
    assert steps >= 100000, steps


def test_a_component_at_inf_is_skipped_by_the_model_too():
    rng = np.random.default_rng(3)
    block = rng.normal(0, 1, (33, 9, 2)).astype(F)
    keep = block.copy()
    u = rng.uniform(-0.5, 0.5, (9, 2)).astype(F)
    out = model.limit(block, u, (0.1, -0.1), (-1, 1), (-1, 1), (np.inf, 0.5), 0.1)
    assert (out[..., 0].view(np.uint32) == block[..., 0].view(np.uint32)).all()
    assert (out[..., 1] != block[..., 1]).any()
    assert (block.view(np.uint32) == keep.view(np.uint32)).all(), "the input is left as it is"
    both = model.limit(block, u, (0.1, -0.1), (-1, 1), (-1, 1), np.inf, 0.1)
    assert (both.view(np.uint32) == block.view(np.uint32)).all()


def test_the_header_takes_the_limits_the_model_takes(header):
    values = np.array([np.nan, 0.0, -1.0, -np.inf, 2.0 ** -149, 1.0, np.inf], dtype=F)
    want = [0, 0, 0, 0, 1, 1, 1]
    assert list(header.valid(values)) == want
    assert list(model.valid(values).astype(int)) == want


RANGES = [((0.0, 1.0), (-np.pi, np.pi)), ((0.2, 1.5), (-2.0, -0.25)), ((-3.0, -1.0), (0.5, 0.75)), ((-1.0, 2.0), (-0.5, 0.5))]


@pytest.mark.parametrize("vrange,wrange", RANGES)
def test_every_limited_sequence_and_every_weighted_mean_is_feasible(vrange, wrange):
    """Random blocks, u inside the box, anchors inside and outside it: what the rollouts re-form from the limited block,
    clip(float32(u + e')), is feasible within tol, the step from the anchor included; and so is the update's
    clip(float32(u + float32(sum(w e') / sum(w)))) with the mean in float64 -- for random positive weights and for one
    weight carrying nearly everything."""
    rng = np.random.default_rng(5)
    n, t = 512, 40
    for trial, (accel, dt) in enumerate([((1.0, 2.0), 0.1), ((0.05, 30.0), 0.1), ((4.0, 0.5), 0.02)]):
        tol = model.tolerance(vrange, wrange, accel, dt)
        u = np.stack([rng.uniform(lo, hi, t) for lo, hi in (vrange, wrange)], axis=1).astype(F)
        u = np.stack([model.clip(u[:, c], *r) for c, r in enumerate((vrange, wrange))], axis=1)  # (float32 of the ends)
        anchor = [rng.uniform(lo - 1, hi + 1) for lo, hi in (vrange, wrange)] if trial else [np.mean(vrange), np.mean(wrange)]
        block = (rng.normal(0, 1, (n, t, 2)) * [0.6, 1.5]).astype(F)
        limited = model.limit(block, u, anchor, vrange, wrange, accel, dt)
        q = model.applied(limited, u, vrange, wrange)
        worst = model.excess(q, anchor, vrange, wrange, accel, dt)
        assert (worst <= tol).all(), (trial, worst, tol)
        # (the unlimited block is not, in the components whose step is shorter than the box: the test shows something)
        binds = model.step_size(accel, dt) < np.array([vrange[1] - vrange[0], wrange[1] - wrange[0]])
        unlimited = model.excess(model.applied(block, u, vrange, wrange), anchor, vrange, wrange, accel, dt)
        assert binds.any() and (unlimited[binds] > 10 * tol[binds]).all()
        heavy = np.full(n, 1e-12)
        heavy[7] = 1.0
        for w in (rng.uniform(0.0, 1.0, n) + 1e-9, np.exp(-rng.uniform(0, 40, n)), heavy):
            mean = np.einsum("n,ntc->tc", w, limited.astype(np.float64)) / w.sum()
            new = np.stack([model.clip(np.add(u[:, c], mean[:, c].astype(F), dtype=F), *r) for c, r in enumerate((vrange, wrange))], axis=1)
            worst = model.excess(new, anchor, vrange, wrange, accel, dt)
            assert (worst <= tol).all(), (trial, worst, tol)
