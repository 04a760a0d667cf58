"""Time-correlated control noise on the host: the numpy model of the recurrence (tests/noise_smoothing_model.py) against
its own edge cases, against csrc/noise_smooth.h compiled with g++ on its own -- the step and the gain the kernel calls --
and against the statistics the recurrence promises (unit variance at every step, lag-1 correlation beta)."""
import os
import subprocess

import numpy as np
import pytest

import noise_smoothing_model as model

HEADER = os.path.join(os.path.dirname(__file__), "..", "mppi_numba_amd", "csrc", "noise_smooth.h")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "%s"
static float as_float(uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; }
static uint32_t as_bits(float f) { uint32_t bits; std::memcpy(&bits, &f, 4); return bits; }
int main() {
  uint32_t in[3];
  while (std::fread(in, 4, 3, stdin) == 3) {
    const float beta = as_float(in[0]), e = as_float(in[1]), w = as_float(in[2]);
    const float g = mppi::noise_smooth_gain(beta);
    const uint32_t out[3] = {as_bits(g), as_bits(mppi::noise_smooth_step(beta, g, e, w)),
                             (uint32_t)mppi::noise_smooth_beta_valid(beta)};
    std::fwrite(out, 4, 3, stdout);
  }
  return 0;
}
"""


def test_beta_zero_and_a_single_step_return_the_input():
    rng = np.random.default_rng(0)
    w = rng.normal(0, 1, (37, 9, 2)).astype(np.float32)
    keep = w.copy()
    out = model.smooth(w, 0.0)
    assert (out.view(np.uint32) == w.view(np.uint32)).all()
    assert (w.view(np.uint32) == keep.view(np.uint32)).all(), "the input is left as it is"
    one = w[:, :1]
    assert (model.smooth(one, (0.9, 0.5)).view(np.uint32) == one.view(np.uint32)).all()
    # one component filtered, the other not
    mixed = model.smooth(w, (0.0, 0.7))
    assert (mixed[..., 0].view(np.uint32) == w[..., 0].view(np.uint32)).all()
    assert (mixed[:, 1:, 1] != w[:, 1:, 1]).any()
    assert model.gain(0.0) == np.float32(1.0) and model.gain(np.float32(0.6)) == np.float32(np.sqrt(1.0 - np.float64(np.float32(0.6)) ** 2))


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("noise_smooth")
    src = tmp / "step.cpp"
    src.write_text(PROGRAM % os.path.abspath(HEADER))
    exe = tmp / "step"
    # -O2 with fused multiply-add available to the compiler: the header must not let it contract the step
    flags = ["-O2", "-ffp-contract=fast"] + (["-mfma"] if os.uname().machine in ("x86_64", "AMD64") else [])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", str(exe), str(src)])

    def run(beta, e, w):
        triples = np.ascontiguousarray(np.stack([beta, e, w], axis=1), dtype=np.float32)
        raw = subprocess.run([str(exe)], input=triples.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        out = np.frombuffer(raw, dtype=np.uint32).reshape(-1, 3)
        assert len(out) == len(triples)
        return out[:, 0].view(np.float32), out[:, 1].view(np.float32), out[:, 2]
    return run


def triples():
    """(beta, e, w): random coefficients and values, coefficients next to 1 and below 2^-12, products that are denormal,
    and the corners."""
    rng = np.random.default_rng(1)
    n = 120000
    beta = rng.uniform(0, 1, n).astype(np.float32)
    beta[beta >= 1.0] = np.float32(0.5)
    e = rng.normal(0, 1, n).astype(np.float32)
    w = rng.normal(0, 1, n).astype(np.float32)
    k = 10000
    # next to 1: 1 - m * 2^-24, m = 1 .. (the gain falls to 2^-12 and below: g * w small beside beta * e)
    beta[:k] = (1.0 - np.arange(1, k + 1) * 2.0 ** -24).astype(np.float32)
    # below 2^-12: beta^2 < 2^-24 vanishes beside 1 in float32, not in the float64 the gain is formed in
    beta[k:2 * k] = (rng.uniform(0, 1, k) * 2.0 ** -12).astype(np.float32)
    beta[2 * k:2 * k + 4] = [0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -13]
    # denormal products: beta * e and g * w below 2^-126
    beta[3 * k:4 * k] = (rng.uniform(0, 1, k) * 2.0 ** -20).astype(np.float32)
    e[3 * k:4 * k] = (rng.normal(0, 1, k) * 2.0 ** -115).astype(np.float32)
    w[3 * k:4 * k] = (rng.normal(0, 1, k) * 2.0 ** -128).astype(np.float32)
    beta[4 * k:5 * k] = (1.0 - np.arange(1, k + 1) * 2.0 ** -24).astype(np.float32)
    w[4 * k:5 * k] = (rng.normal(0, 1, k) * 2.0 ** -118).astype(np.float32)
    e[4 * k:5 * k] = (rng.normal(0, 1, k) * 2.0 ** -127).astype(np.float32)
    # sums that cancel, where a fused product would show
    e[5 * k:6 * k] = -w[5 * k:6 * k]
    assert ((beta >= 0) & (beta < 1)).all()
    return beta, e, w


def test_the_header_agrees_with_the_model_bit_for_bit(header):
    beta, e, w = triples()
    assert len(beta) >= 100000
    got_gain, got_step, valid = header(beta, e, w)
    want_gain = model.gain(beta)
    want_step = model.step(beta, want_gain, e, w)
    assert valid.all()
    assert (got_gain.view(np.uint32) == want_gain.view(np.uint32)).all()
    bad = got_step.view(np.uint32) != want_step.view(np.uint32)
    assert not bad.any(), "%d of %d steps differ, first (beta, e, w) = %s" % (
        bad.sum(), bad.size, (beta[bad][:1], e[bad][:1], w[bad][:1]))
    # the triples reach what they are there for
    products = np.abs(np.multiply(beta, e, dtype=np.float32))
    assert ((products > 0) & (products < 2.0 ** -126)).sum() >= 1000, "denormal products"
    assert (want_gain < 2.0 ** -11).sum() >= 1 and (want_gain == 1.0).sum() >= 5000
    # ... and a fused step would not have passed: on the cancelling sums it differs from the model somewhere
    fused = (beta.astype(np.float64) * e.astype(np.float64) + np.multiply(want_gain, w, dtype=np.float32).astype(np.float64)).astype(np.float32)
    assert (fused.view(np.uint32) != want_step.view(np.uint32)).any()


def test_the_header_refuses_what_the_recurrence_does_not_take(header):
    beta = np.array([1.0, -0.1, np.nan, np.inf, -np.inf, np.float32(1 - 2.0 ** -25), 1.5, 0.0, -0.0, 0.999], dtype=np.float32)
    zero = np.zeros_like(beta)
    _, _, valid = header(beta, zero, zero)
    assert list(valid) == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1]  # (float32(1 - 2^-25) is 1)


@pytest.mark.parametrize("beta", [0.9, 0.5])
def test_every_step_keeps_its_variance_and_the_lag_one_correlation_is_beta(beta):
    """N = 4096, T = 50: the per-step standard deviation over 4096 samples has a standard error of 1 / sqrt(2 * 4096) =
    1.1 %, the bound is 5 %; the pooled lag-1 correlation over 49 * 4096 = 2e5 pairs has a standard error below 0.003,
    the bound is 0.02."""
    w = np.random.default_rng(7).normal(0, 1, (4096, 50, 2)).astype(np.float32)
    e = model.smooth(w, beta).astype(np.float64)
    std = e.std(axis=0)
    assert np.abs(std - 1.0).max() < 0.05, std
    for c in range(2):
        a, b = e[:, :-1, c].ravel(), e[:, 1:, c].ravel()
        corr = np.corrcoef(a, b)[0, 1]
        assert abs(corr - beta) < 0.02, (c, corr)
