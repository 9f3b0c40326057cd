"""The crafted RSA encodings and length sweeps of tests/craft.py on the device:
every single-byte deviation of the PKCS#1 v1.5 EM, every PSS salt length and
reject rule (2047- to 4096-bit keys, all three hashes), correctly signed
signing inputs of every length 1..300 (and around SMALL_IN_MAX), EdDSA inputs
around the SHA-512 block edges -- each through
  1. one batch: the chain k_prep -> k_rsa_modexp -> k_rsa_pad (k_ed_* for EdDSA),
  2. the chain again in calls of 7 (other wave fill, other arena offsets),
  3. the one-launch paths k_rsa_small / k_ed_small in calls of at most 64
     (kernels/small_common.hpp sm_stage_input / sm_hash and the small EM compare),
with the arena offsets of the jobs walking through all alignments mod 4.  Every
verdict must equal the C oracle's (tests/test_rsa_em_reference.py pins the
oracle to the plain-Python restatement of the Go rule and to the construction)."""
import pytest

from oracle import jws
from tests import craft

pytestmark = pytest.mark.gpu

KIDS = craft.RSA_KIDS + ["ed-a"]
KID_INDEX = {kid: i for i, kid in enumerate(KIDS)}
SMALL_RSA_KIDS = ("rsa2047-a", "rsa2048-a", "rsa2049-b")       # the RSA-2K class (k_rsa_small)


@pytest.fixture(scope="module")
def cases():
    return craft.cases()[0]


@pytest.fixture(scope="module")
def want(cases):
    K = craft.keys()
    okeys = {}
    for kid in KIDS:
        k = K[kid]
        okeys[kid] = jws.Key("OKP", kid, crv="Ed25519", x=craft.ed_public(k)[2]) if kid == "ed-a" else \
            jws.Key("RSA", kid, n=k.n.to_bytes(k.k, "big"), e=k.e)
    w = [int(jws.verify_alg_sig(alg, okeys[kid], msg, sig)) for _, alg, kid, msg, sig, _ in cases]
    assert w == [c[5] for c in cases]
    assert sum(w) > 1000 and len(w) - sum(w) > 1000
    return w


@pytest.fixture(scope="module")
def ctx():
    from cap_amd import _lib
    K = craft.keys()
    c = _lib.Context()
    keys = [_lib.Key.rsa(K[kid].n.to_bytes(K[kid].k, "big"), K[kid].e) for kid in craft.RSA_KIDS]
    keys.append(_lib.Key.ed25519(craft.ed_public(K["ed-a"])[2]))
    c.load_keys(keys)
    yield c
    c.close()


def _verify(ctx, cases, idx, per_call):
    """verdicts of cases[i] for i in idx, `per_call` jobs a call; job i starts
    i % 4 bytes further into the arena, so offsets take every alignment"""
    from cap_amd import _lib
    out, calls = [], 0
    for lo in range(0, len(idx), per_call):
        arena = _lib.Arena()
        for i in idx[lo:lo + per_call]:
            _, alg, kid, msg, sig, _ = cases[i]
            arena.buf += b"#" * (i % 4)
            arena.add(msg, jws.b64url_encode(sig).encode(), alg, KID_INDEX[kid])
        out += list(ctx.verify(arena))
        calls += 1
    return out, calls


def _diff(cases, idx, got, want):
    return [(cases[i][0], g, want[i]) for i, g in zip(idx, got) if g != want[i]]


def test_chain_one_batch(ctx, cases, want):
    idx = list(range(len(cases)))
    n0 = ctx.debug_small_path()
    got, _ = _verify(ctx, cases, idx, len(idx))
    assert ctx.debug_small_path() == n0
    bad = _diff(cases, idx, got, want)
    assert not bad, (len(bad), bad[:12])


def test_chain_calls_of_seven(ctx, cases, want):
    idx = list(range(len(cases)))
    ctx.debug_small_path(False)
    try:
        n0 = ctx.debug_small_path()
        got, _ = _verify(ctx, cases, idx, 7)
        assert ctx.debug_small_path() == n0
    finally:
        ctx.debug_small_path(True)
    bad = _diff(cases, idx, got, want)
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("per_call", [64, 5])
def test_rsa_small_path(ctx, cases, want, per_call):
    """RS256 / RS384 / RS512 on the RSA-2K keys: k_rsa_small, one launch a call."""
    idx = [i for i, c in enumerate(cases) if c[2] in SMALL_RSA_KIDS and c[1].startswith("RS")
           and len(c[3]) <= craft.SMALL_IN_MAX]
    if per_call != 64:
        idx = idx[::3]
    assert len(idx) >= 400
    n0 = ctx.debug_small_path()
    got, calls = _verify(ctx, cases, idx, per_call)
    assert ctx.debug_small_path() - n0 == calls
    bad = _diff(cases, idx, got, want)
    assert not bad, (len(bad), bad[:12])


def test_rsa_input_past_small_limit_takes_the_chain(ctx, cases, want):
    idx = [i for i, c in enumerate(cases) if len(c[3]) > craft.SMALL_IN_MAX]
    assert [cases[i][0] for i in idx] == [f"len/RS256/{craft.SMALL_IN_MAX + 1}"]
    n0 = ctx.debug_small_path()
    got, _ = _verify(ctx, cases, idx, 1)
    assert ctx.debug_small_path() == n0
    assert got == [want[i] for i in idx] == [1]


@pytest.mark.parametrize("per_call", [64, 1])
def test_eddsa_sweep_small_path(ctx, cases, want, per_call):
    idx = [i for i, c in enumerate(cases) if c[1] == "EdDSA"]
    assert len(idx) == 107
    n0 = ctx.debug_small_path()
    got, calls = _verify(ctx, cases, idx, per_call)
    assert ctx.debug_small_path() - n0 == calls
    bad = _diff(cases, idx, got, want)
    assert not bad, (len(bad), bad[:12])
