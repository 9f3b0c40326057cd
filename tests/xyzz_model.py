"""Big-integer side of the XYZZ accumulator tests (kernels/ecdsa_impl.hpp
madd_xyzz / madd_xyzz_z1, the addition chain of k_ec_point for P-256).

The device hook tk_ec_xyzz_chain (cap_amd/csrc/tests/tk_ec_xyzz.hip) takes, per
lane, affine points as canonical Montgomery 28-bit limbs with a sign each and
returns (X, Y, ZZ, ZZZ).  This module builds the lanes, computes what the sum
must be in Python integers, and checks a lane's output against it:

    x = X / ZZ and y = Y / ZZZ equal the sum,  ZZ^3 == ZZZ^2,  ZZ != 0;
    for a lane with a step that adds P to P or to -P: ZZ == ZZZ == 0 (mod p)
    from that step on, whatever is added afterwards.

The reference is the chord rule on affine integers, lambda = (y2 - y1) /
(x2 - x1), x3 = lambda^2 - x1 - x2, y3 = lambda (x1 - x3) - y1.  It does not
read the curve's b, and neither does the mixed addition, so the lanes that
put coordinates at the limb extremes need not lie on the curve; the random
lanes do (multiples of G), and their sums are cross-checked against the scalar
multiple table_model.ec_mul gives.

xyzz_chain is the device's formulas (EFD madd-2008-s) in integers.  It is not
the reference: tests/test_xyzz_model.py runs it through check_lane to show that
the check passes on a correct chain and fails on a wrong sign, in the
reference's inputs or in the formulas."""
import random

from tests import table_model as T

CLS = T.CLS_P256
P = T.EC[CLS]["p"]
L = T.EC[CLS]["L"]
W = T.LIMB_BITS
R = 1 << (W * L)
RINV = pow(R, -1, P)
MASK = (1 << W) - 1
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
OUT_WORDS = 4 * L + 1
STEPS = 26                                   # the longest lane: an exceptional step at 20 and five more

# coordinates at the limb extremes, as the Montgomery values the kernel sees
EXTREMES = [P - 1, 1, 2**256 - 2**224,
            (0xe << (W * (L - 1))) | ((1 << (W * (L - 1))) - 1),      # every 28-bit limb below the top all ones
            sum(MASK << (W * j) for j in range(0, L - 1, 2)),          # alternate limbs all ones
            0]
assert all(0 <= v < P for v in EXTREMES)


def limbs(v):
    assert 0 <= v < P
    return [(v >> (W * j)) & MASK for j in range(L)]


def value(ls):
    return sum(int(x) << (W * j) for j, x in enumerate(ls))


def to_mont(v):
    return v * R % P


def from_mont(v):
    return v * RINV % P


def neg(pt):
    return pt[0], -pt[1] % P


def chord(p1, p2):
    """p1 + p2 by the chord rule; None where x1 == x2 (p2 == +-p1: the exceptional pair)"""
    if p1[0] == p2[0]:
        return None
    lam = (p2[1] - p1[1]) * pow(p2[0] - p1[0], -1, P) % P
    x3 = (lam * lam - p1[0] - p2[0]) % P
    return x3, (lam * (p1[0] - x3) - p1[1]) % P


def reference(points, signs):
    """the sum of sign * point over the steps (sign 0: skipped), by the chord
    rule: (affine point or None if nothing was added, exceptional)"""
    acc = None
    for pt, s in zip(points, signs):
        if s == 0:
            continue
        q = pt if s > 0 else neg(pt)
        if acc is None:
            acc = q
            continue
        acc = chord(acc, q)
        if acc is None:
            return None, True
    return acc, False


def xyzz_chain(points, signs, r_sign=-1):
    """The device's chain in plain integers mod p: assignment, then madd-2008-s
    (the Z = 1 form is the same formulas with ZZ = ZZZ = 1).  r_sign = +1
    injects a wrong sign into r = S2 - Y.  Returns (X, Y, ZZ, ZZZ, empty)."""
    X = Y = ZZ = ZZZ = 0
    empty = True
    for (x2, y2), s in zip(points, signs):
        if s == 0:
            continue
        if s < 0:
            y2 = -y2 % P
        if empty:
            X, Y, ZZ, ZZZ, empty = x2, y2, 1, 1, False
            continue
        u2, s2 = x2 * ZZ % P, y2 * ZZZ % P
        h, r = (u2 - X) % P, (s2 + r_sign * Y) % P
        hh = h * h % P
        hhh, v = h * hh % P, X * hh % P
        ZZ, ZZZ = ZZ * hh % P, ZZZ * hhh % P
        X3 = (r * r - hhh - 2 * v) % P
        X, Y = X3, (r * (v - X3) - Y * hhh) % P
    return X, Y, ZZ, ZZZ, empty


class Lane:
    def __init__(self, tag, points, signs, scalar=None):
        """points: affine plain integers (x, y); signs: +1 / -1 / 0 per step;
        scalar: sum sign_i k_i where every point is k_i G (cross-check)"""
        assert len(points) == len(signs) <= STEPS
        self.tag, self.points, self.signs, self.scalar = tag, points, signs, scalar
        self.want, self.exceptional = reference(points, signs)


def check_lane(lane, X, Y, ZZ, ZZZ, empty):
    """X, Y, ZZ, ZZZ: plain integers (the device's Montgomery values times R^-1),
    any representative mod p.  Raises AssertionError on a mismatch."""
    t = lane.tag
    X, Y, ZZ, ZZZ = X % P, Y % P, ZZ % P, ZZZ % P
    if lane.exceptional:
        assert ZZ == 0 and ZZZ == 0, (t, "an exceptional step must leave ZZ == ZZZ == 0")
        return
    if lane.want is None:
        assert empty, (t, "nothing added")
        return
    assert not empty, t
    assert ZZ != 0 and ZZZ != 0, (t, "ZZ == 0 without an exceptional step")
    assert pow(ZZ, 3, P) == ZZZ * ZZZ % P, (t, "ZZ^3 != ZZZ^2")
    got = X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P
    assert got == lane.want, (t, "sum", got, lane.want)
    if lane.scalar is not None:
        k = lane.scalar % N
        assert k != 0
        assert got == T.ec_mul(CLS, k, T.ec_generator(CLS)), (t, "scalar multiple")


def mont_point(vx, vy):
    """the affine point whose Montgomery coordinates are the values vx, vy"""
    return from_mont(vx), from_mont(vy)


def build_lanes(seed=0xEC22):
    """At most 64 lanes (one wave).  Chains of 1, 2, 3 and 20 additions are
    where the assignment, the Z = 1 form and the general form first appear."""
    rng = random.Random(seed)
    G = T.ec_generator(CLS)
    ks = [rng.randrange(1, N) for _ in range(32)]
    pool = [T.ec_mul(CLS, k, G) for k in ks]
    lanes = []

    def rand_lane(tag, n, signs=None):
        idx = rng.sample(range(len(pool)), n)
        sg = list(signs) + [rng.choice((1, -1)) for _ in range(n - len(signs))] if signs else \
            [rng.choice((1, -1)) for _ in range(n)]
        lanes.append(Lane(tag, [pool[i] for i in idx], sg, sum(s * ks[i] for s, i in zip(sg, idx))))

    for n in (1, 2, 3, 20):
        for rep in range(2):
            rand_lane(f"random n={n} #{rep}", n)
    # every sign pattern of the first three steps, alone and ahead of a long chain
    for m in range(8):
        sg = [1 if (m >> b) & 1 else -1 for b in range(3)]
        rand_lane(f"signs {sg}", 3, sg)
        rand_lane(f"signs {sg} then 17 more", 20, sg)
    # a skipped step (a zero digit) in each position
    for z in range(3):
        sg = [1, -1, 1, 1]
        sg[z] = 0
        rand_lane(f"zero sign at step {z}", 4, sg)
    # coordinates at the limb extremes (Montgomery values), as the assigned
    # entry, the entry of the Z = 1 form and the entry of the general form
    ext = [(a, b) for a in EXTREMES for b in EXTREMES if a != b][::3]
    for i, (vx, vy) in enumerate(ext[:10]):
        e = mont_point(vx, vy)
        o1, o2 = pool[i], pool[i + 1]
        where = i % 3
        pts = [o1, o2, pool[i + 2]]
        pts[where] = e
        sg = [1, -1 if i & 1 else 1, -1 if i & 2 else 1]
        lanes.append(Lane(f"extreme x={vx:#x} y={vy:#x} at step {where}", pts, sg))
    lanes.append(Lane("extremes in every step", [mont_point(EXTREMES[0], EXTREMES[1]), mont_point(EXTREMES[2], EXTREMES[3]),
                                                 mont_point(EXTREMES[1], EXTREMES[0]), mont_point(EXTREMES[3], EXTREMES[4])],
                      [1, -1, -1, 1]))
    # exceptional steps: the entry is the accumulator itself (P + P) or its
    # negative (P - P), in the Z = 1 form (step 1) and in the general form
    # (steps 2 and 20), each followed by five further additions
    for at in (1, 2, 20):
        for sgn, name in ((1, "P + P"), (-1, "P - P")):
            idx = rng.sample(range(len(pool)), at + 5)
            pts = [pool[i] for i in idx[:at]]
            sg = [rng.choice((1, -1)) for _ in range(at)]
            acc, exc = reference(pts, sg)
            assert not exc
            lanes.append(Lane(f"{name} at step {at}, five more", pts + [acc] + [pool[i] for i in idx[at:]],
                              sg + [sgn] + [rng.choice((1, -1)) for _ in range(5)]))
            assert lanes[-1].exceptional
    assert len(lanes) <= 64
    return lanes


def pack(lanes):
    """the hook's arrays: (points as n x STEPS x 2L limbs, signs, counts), flat lists"""
    pts, sg, cnt = [], [], []
    for ln in lanes:
        for (x, y), s in zip(ln.points, ln.signs):
            pts += limbs(to_mont(x)) + limbs(to_mont(y))
            sg.append(s)
        pad = STEPS - len(ln.points)
        pts += [0] * (2 * L * pad)
        sg += [0] * pad
        cnt.append(len(ln.points))
    return pts, sg, cnt
