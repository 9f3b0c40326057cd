"""The crafted RSA encodings of tests/craft.py (every single-byte deviation of
EMSA-PKCS1-v1_5, every PSS salt length and reject rule, signing inputs of every
length) against two references that share no code: craft.em_accepts, a plain
hashlib restatement of Go's rsa.VerifyPKCS1v15 / rsa.VerifyPSS(auto salt) on
EM = s^e mod n, and the C oracle's verify_alg_sig.  Both must give the verdict
each case was built for.  tests/test_gpu_rsa_em.py runs the same list on the
device; this test pins the references to each other without one."""
import pytest

from oracle import jws
from tests import craft


@pytest.fixture(scope="module")
def cases():
    return craft.cases()


def _okey(kid):
    k = craft.keys()[kid]
    if kid == "ed-a":
        return jws.Key("OKP", kid, crv="Ed25519", x=craft.ed_public(k)[2])
    return jws.Key("RSA", kid, n=k.n.to_bytes(k.k, "big"), e=k.e)


def test_case_list_shape(cases):
    cs, skipped = cases
    cnt = craft.summary(cs)
    print("crafted cases:", len(cs), "skipped (EM >= n):", list(skipped))
    for key in sorted(cnt):
        print("  ", *key, cnt[key])
    names = [c[0] for c in cs]
    assert len(set(names)) == len(names)
    k2 = craft.keys()["rsa2048-a"]
    # the dense lists are whole: both flips of every EM byte but the unsignable ones, every salt length
    flips = [n for n in names if n.startswith("rsa2048-a/RS256/flip")]
    assert len(flips) + sum(s.startswith("rsa2048-a/RS256/flip") for s in skipped) == 2 * k2.k
    for hbits in (256, 384, 512):
        assert sum(n.startswith(f"rsa2048-a/PS{hbits}/salt") for n in names) == k2.k - hbits // 8 - 2 + 1
    assert sum(n.startswith("len/RS256/") for n in names) == 303
    assert sum(n.startswith("len/EdDSA/") for n in names) == 107
    # the key sizes the lists are for: k % 4 == 1 and emLen == k - 1 on the 2049-bit key (the PSS
    # lead byte), 8 emLen - emBits == 2 on the 2047-bit key (two masked-out top bits)
    K = craft.keys()
    assert [K[kid].bits for kid in craft.RSA_KIDS] == [2047, 2048, 2049, 3072, 4096]
    assert K["rsa2049-b"].k == 257
    for hbits in (256, 384, 512):
        assert f"rsa2049-b/PS{hbits}/lead-nonzero" in names
        assert f"rsa2047-a/PS{hbits}/topbit6" in names or f"rsa2047-a/PS{hbits}/topbit6" in skipped
    # a skipped case is a mutation of the top EM byte(s) only (craft.cases asserts it per case)
    assert len(skipped) <= 12
    assert {c[2] for c in cs} == set(craft.RSA_KIDS) | {"ed-a"}


def test_em_reference_equals_oracle_and_construction(cases):
    cs, _ = cases
    bad = []
    for name, alg, kid, msg, sig, expected in cs:
        orc = int(jws.verify_alg_sig(alg, _okey(kid), msg, sig))
        if alg == "EdDSA":
            ref = expected                    # no EM: the oracle alone checks the signer
        else:
            k = craft.keys()[kid]
            em = pow(int.from_bytes(sig, "big"), k.e, k.n).to_bytes(k.k, "big")
            ref = int(craft.em_accepts(alg, k.bits, em, msg))
        if not ref == orc == expected:
            bad.append((name, ref, orc, expected))
    assert not bad, (len(bad), bad[:10])


def test_em_reference_rejects_wrong_length_and_alg():
    """em_accepts on its own edges: EM of another length, the PKCS#1 EM under a PS alg and back."""
    k = craft.keys()["rsa2048-a"]
    msg = b"abc"
    em = craft.pkcs1_em(k.k, 256, msg)
    assert craft.em_accepts("RS256", k.bits, em, msg)
    assert not craft.em_accepts("RS256", k.bits, em[1:], msg)
    assert not craft.em_accepts("RS384", k.bits, em, msg)
    assert not craft.em_accepts("PS256", k.bits, em, msg)
    pem = craft.pss_em(k.bits, 256, msg, b"salt")
    assert craft.em_accepts("PS256", k.bits, pem, msg)
    assert not craft.em_accepts("PS512", k.bits, pem, msg)
    assert not craft.em_accepts("RS256", k.bits, pem, msg)
    assert not craft.em_accepts("PS256", k.bits, pem, msg + b"d")
