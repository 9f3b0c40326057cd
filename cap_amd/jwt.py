"""cap's jwt package API, backed by the MI355X verifier.

Mirrors the Go reference one to one (same names, argument meaning, error
strings); every call goes to the C++ host mirror (cap_amd/csrc/host/cap_jwt.hpp)
and every signature check to libcapjwt.so on the GPU.  Go's `(value, error)`
returns become `(value, err)` tuples with `err` a str or None.

    Go (reference)                                  here
    jwt.NewStaticKeySet      jwt/keyset.go:142       NewStaticKeySet
    jwt.NewJSONWebKeySet     jwt/keyset.go:109       NewJSONWebKeySet
    jwt.NewOIDCDiscoveryKeySet jwt/keyset.go:49      NewOIDCDiscoveryKeySet
    KeySet.VerifySignature   jwt/keyset.go:27-32     KeySet.VerifySignature (+ VerifySignatureBatch)
    jwt.ParsePublicKeyPEM    jwt/keyset.go:178       ParsePublicKeyPEM
    jwt.NewValidator         jwt/jwt.go:25           NewValidator
    Validator.Validate       jwt/jwt.go:95           Validator.Validate (+ ValidateBatch, north star)
    (verdict only)                                   Validator.CheckBatch / CheckBlob: Validate's error per
                                                     token, registered claims scanned on the GPU, no claims map
    (verdict + named claims)                         Validator.RegisteredBatch / SelectBatch (+ Blob forms):
                                                     jwt.Claims and caller-named claims from the same scan
    (verdict + yes/no questions)                     Validator.MatchBatch / MatchBlob with Equals, HasWord,
                                                     HasElement, Present: a mask per token from the same scan
    jwt.Expected             jwt/jwt.go:38           Expected
    jwt.SupportedSigningAlgorithm jwt/algs.go:38     SupportedSigningAlgorithm

HTTP is the caller's: NewJSONWebKeySet / NewOIDCDiscoveryKeySet take a
`fetch(url, ca_pem) -> {"status", "body", "content_type", "max_age"}` callable
standing in for the reference's net/http client (raise for a transport error).
"""
import array
import dataclasses
import datetime
from typing import Callable, List, Optional, Sequence

from . import _lib  # noqa: F401  (loads libcapjwt.so first; fails loudly if missing)
from . import _capjwt_host as _h

# jwt/algs.go:12-21
RS256, RS384, RS512 = "RS256", "RS384", "RS512"
ES256, ES384, ES512 = "ES256", "ES384", "ES512"
PS256, PS384, PS512 = "PS256", "PS384", "PS512"
EdDSA = "EdDSA"
DefaultLeewaySeconds = 150          # jwt/jwt.go:16

PublicKey = _h.PublicKey


def SupportedSigningAlgorithm(*algs) -> Optional[str]:
    """jwt/algs.go:38-46: None, or `unsupported signing algorithm "X"`."""
    return _h.supported_signing_algorithm(list(algs))


def ParsePublicKeyPEM(data):
    """jwt/keyset.go:178-200 -> (PublicKey, err)."""
    try:
        return _h.parse_public_key_pem(data if isinstance(data, bytes) else data.encode()), None
    except ValueError as e:
        return None, str(e)


class KeySet:
    """jwt.KeySet (jwt/keyset.go:27-32), GPU-backed."""

    def __init__(self, impl):
        self._impl = impl

    def VerifySignature(self, token, ctx=None):
        return tuple(self._impl.verify_signature(token))

    def WaitTables(self):
        """Block until the key comb tables of the last key (re)load reach their
        budgeted width (keys verify before that, on narrower tables)."""
        self._impl.wait_tables()

    def VerifySignatureBatch(self, tokens: Sequence, ctx=None):
        return [tuple(r) for r in self._impl.verify_signature_batch(list(tokens))]

    def SetCoalescing(self, max_inflight=4, max_batch=65536, window_us=0):
        """Batching of concurrent single-token calls (VerifySignature and
        Validator.Validate): at most `max_inflight` device batches at once, each
        of at most `max_batch` tokens, collected for at most `window_us`.  The
        defaults are the library's (host/cap_jwt.hpp CoalesceConfig)."""
        self._impl.set_coalescing(int(max_inflight), int(max_batch), int(window_us))

    def CoalescingStats(self):
        return dict(self._impl.coalescing_stats())

    def DeviceStatus(self) -> str:
        """"" while the GPU context verifies; else why it is lost (it is
        recreated after a device error; see DeviceRecoveries)."""
        return self._impl.device_status()

    def DeviceRecoveries(self) -> int:
        return self._impl.device_recoveries()


def NewStaticKeySet(public_keys: List, devices=()):
    try:
        return KeySet(_h.new_static_keyset(list(public_keys), list(devices))), None
    except ValueError as e:
        return None, str(e)


def NewJSONWebKeySet(ctx, jwks_url: str, jwks_ca_pem: str = "", fetch: Callable = None, devices=()):
    try:
        return KeySet(_h.new_json_web_keyset(jwks_url, jwks_ca_pem, fetch, list(devices))), None
    except ValueError as e:
        return None, str(e)


def NewOIDCDiscoveryKeySet(ctx, issuer: str, issuer_ca_pem: str = "", fetch: Callable = None, devices=()):
    try:
        return KeySet(_h.new_oidc_discovery_keyset(issuer, issuer_ca_pem, fetch, list(devices))), None
    except ValueError as e:
        return None, str(e)


def _dur_ns(d) -> int:
    """time.Duration from a timedelta or a number of seconds."""
    if d is None:
        return 0
    if isinstance(d, datetime.timedelta):
        return (d.days * 86400 + d.seconds) * 1_000_000_000 + d.microseconds * 1000
    return int(round(d * 1e9))


def _time_ns(t) -> int:
    if isinstance(t, datetime.datetime):
        if t.tzinfo is None:
            t = t.replace(tzinfo=datetime.timezone.utc)
        d = t - datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
        return _dur_ns(d)
    return int(round(t * 1e9))


@dataclasses.dataclass
class Expected:
    """jwt/jwt.go:38-83.  Leeways: timedelta or seconds; Now: callable returning
    a datetime or unix seconds (None -> time.Now())."""
    Issuer: str = ""
    Subject: str = ""
    ID: str = ""
    Audiences: List[str] = dataclasses.field(default_factory=list)
    SigningAlgorithms: List[str] = dataclasses.field(default_factory=list)
    NotBeforeLeeway: object = 0
    ExpirationLeeway: object = 0
    ClockSkewLeeway: object = 0
    Now: Optional[Callable] = None

    def _native(self):
        e = _h.Expected()
        e.Issuer, e.Subject, e.ID = self.Issuer, self.Subject, self.ID
        e.Audiences = list(self.Audiences or [])
        e.SigningAlgorithms = list(self.SigningAlgorithms or [])
        e.NotBeforeLeeway = _dur_ns(self.NotBeforeLeeway)
        e.ExpirationLeeway = _dur_ns(self.ExpirationLeeway)
        e.ClockSkewLeeway = _dur_ns(self.ClockSkewLeeway)
        if self.Now is not None:
            e.has_now = True
            e.now_unix_ns = _time_ns(self.Now())
        return e


class Path(tuple):
    """A claim inside objects, by the keys that lead to it: Path("realm_access",
    "roles") is claims["realm_access"]["roles"].  An element of the `names` of
    SelectBatch / SelectBlob and their *Each forms.  Every component is a literal
    key (str): nothing in it is parsed as a separator, and "a.b" stays one key."""

    def __new__(cls, *components):
        if not components:
            raise ValueError("Path: at least one component")
        for c in components:
            if not isinstance(c, str):
                raise TypeError("Path: components are str")
        return super().__new__(cls, components)

    def __repr__(self):
        return "Path(" + ", ".join(repr(c) for c in self) + ")"


def _paths_of(names):
    """None for a list of names alone; else every element as a path (a name is a path of one component)"""
    names = list(names)
    if not any(isinstance(x, Path) for x in names):
        return names, None
    return names, [list(x) if isinstance(x, Path) else [x] for x in names]


class Require(tuple):
    """A yes/no question about one claim, an element of the `requires` of
    MatchBatch / MatchBlob and their *Each forms: (path, op, value).  Built by
    Equals, HasWord, HasElement and Present."""
    EQUALS, HAS_WORD, HAS_ELEMENT, PRESENT = 1, 2, 3, 4          # jg_pred_op (include/jg.h)

    def __new__(cls, path_or_name, op, value=""):
        path = path_or_name if isinstance(path_or_name, Path) else Path(path_or_name)
        if not isinstance(value, str):
            raise TypeError("Require: the value is a str")
        return super().__new__(cls, (path, int(op), value))

    def __repr__(self):
        name = {1: "Equals", 2: "HasWord", 3: "HasElement", 4: "Present"}.get(self[1], "Require")
        return "%s(%r%s)" % (name, self[0], "" if self[1] == self.PRESENT else ", %r" % self[2])


def Equals(path_or_name, v: str) -> Require:
    """The claim is a string equal to v ("" allowed)."""
    return Require(path_or_name, Require.EQUALS, v)


def HasWord(path_or_name, v: str) -> Require:
    """The claim is a string and one of its space-separated words (Go's
    strings.Split(s, " "), the RFC 6749 scope form) equals v."""
    return Require(path_or_name, Require.HAS_WORD, v)


def HasElement(path_or_name, v: str) -> Require:
    """The claim is an array and one of its direct elements is a string equal to v."""
    return Require(path_or_name, Require.HAS_ELEMENT, v)


def Present(path_or_name) -> Require:
    """The claims map holds the claim; null counts."""
    return Require(path_or_name, Require.PRESENT, "")


def _requires_of(requires):
    out = []
    for r in requires:
        if not isinstance(r, Require):
            raise TypeError("requires: elements are built by Equals, HasWord, HasElement or Present")
        out.append((list(r[0]), r[1], r[2]))
    return out


class ArgRequire(tuple):
    """A requirement whose other side is the token's own operand, or a number: an
    element of the `requires` of MatchBatchArgs / MatchBlobArgs and their *Each
    forms, beside Require's: (path, op, "", bound, column).  Built by EqualsEach,
    AtLeast, AtMost, AtLeastEach and AtMostEach."""
    EQUALS_ARG, NUM_GE, NUM_LE, NUM_GE_ARG, NUM_LE_ARG = 5, 6, 7, 8, 9     # jg_pred_op (include/jg.h)
    EQUALS_HASH, IS_STRING = 10, 11
    _NAMES = {5: "EqualsEach", 6: "AtLeast", 7: "AtMost", 8: "AtLeastEach", 9: "AtMostEach", 10: "HashOfEach",
              11: "IsString"}

    def __new__(cls, path_or_name, op, bound=0, column=0):
        path = path_or_name if isinstance(path_or_name, Path) else Path(path_or_name)
        for what, v, lo, hi in (("bound", bound, -(1 << 63), (1 << 63) - 1), ("column", column, 0, (1 << 32) - 1)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError("ArgRequire: the %s is an int" % what)
            if not lo <= v <= hi:
                raise ValueError("ArgRequire: the %s does not fit" % what)
        return super().__new__(cls, (path, int(op), "", bound, column))

    def __repr__(self):
        if self[1] == self.IS_STRING:
            return "IsString(%r)" % (self[0],)
        return "%s(%r, %r)" % (self._NAMES.get(self[1], "ArgRequire"), self[0],
                               self[3] if self[1] in (self.NUM_GE, self.NUM_LE) else self[4])


def EqualsEach(path_or_name, column: int) -> ArgRequire:
    """The claim is a string equal to the token's own entry in string column `column` ("" allowed)."""
    return ArgRequire(path_or_name, ArgRequire.EQUALS_ARG, column=column)


def AtLeast(path_or_name, n: int) -> ArgRequire:
    """The claim is a number f with f >= float64(n), as Go compares a claims map's float64."""
    return ArgRequire(path_or_name, ArgRequire.NUM_GE, bound=n)


def AtMost(path_or_name, n: int) -> ArgRequire:
    """The claim is a number f with f <= float64(n)."""
    return ArgRequire(path_or_name, ArgRequire.NUM_LE, bound=n)


def AtLeastEach(path_or_name, column: int) -> ArgRequire:
    """AtLeast with the token's own entry in number column `column` as n."""
    return ArgRequire(path_or_name, ArgRequire.NUM_GE_ARG, column=column)


def AtMostEach(path_or_name, column: int) -> ArgRequire:
    """AtMost with the token's own entry in number column `column` as n."""
    return ArgRequire(path_or_name, ArgRequire.NUM_LE_ARG, column=column)


def HashOfEach(path_or_name, column: int) -> ArgRequire:
    """The claim is a string equal to base64url(SHA-2(x)[:half]) of the token's own entry x in hash column
    `column`, with the SHA-2 of the token's alg: what at_hash is to the access token and c_hash to the
    authorization code (oidc/id_token.go verifyHashClaim).  Never holds under EdDSA or for a None entry."""
    return ArgRequire(path_or_name, ArgRequire.EQUALS_HASH, column=column)


def IsString(path_or_name) -> ArgRequire:
    """The claim is a string ("" counts; null, numbers, arrays and objects do not)."""
    return ArgRequire(path_or_name, ArgRequire.IS_STRING)


class ClaimSet:
    """A set of strings a claim can be held against: a deny-list of revoked jti, the
    tenants a gateway serves.  Made by Validator.NewClaimSet; it owns one of the 16
    set ids of the validator's key set until Close() (or until it is collected).
    A set all of whose members the device takes -- at most 255 bytes, each printable
    ASCII without quote and backslash -- is resident on the device and asked by the
    scan; any other set is host-only (info()["host_only"]) and every token of a
    call that names it is answered from the host path: no result depends on it."""

    def __init__(self, validator, members, seed=None):
        self._validator = validator                      # the context the set lives in
        self._impl = validator._impl.new_claim_set(_members_of(members), seed)

    def Replace(self, members, seed=None):
        """The whole set anew, under the same id.  A failure (a NUL in a member:
        ValueError; no room on the device: RuntimeError) leaves the old members in force."""
        self._impl.replace(_members_of(members), seed)

    def Add(self, members) -> int:
        """Adds members -> how many were new.  Only those go to the device, where a
        kernel inserts them (no rebuild, no upload of the whole set).  A failure (a NUL
        in a member: ValueError; no room on the device: RuntimeError) leaves the old
        members in force; a member the device does not take turns the set host-only."""
        return self._impl.add(_members_of(members))

    def Close(self):
        """Frees the id now; a later call that names the set raises ValueError."""
        self._impl.close()

    def info(self) -> dict:
        """n, host_only and, of the resident table, nslots, maxprobe, seed, pool_bytes, generation"""
        return dict(self._impl.info())

    def __len__(self):
        return len(self._impl)


def _members_of(members):
    out = []
    for m in members:
        if isinstance(m, (bytes, bytearray)):
            m = bytes(m).decode("utf-8", "surrogateescape")
        elif not isinstance(m, str):
            raise TypeError("ClaimSet: a member is a str")
        out.append(m)
    return out


class SetRequire(tuple):
    """A requirement whose other side is a ClaimSet: (path, op, claim set).  Built by InSet and AnyElementIn."""
    IN_SET, ELEMENT_IN_SET = 12, 13                      # jg_pred_op (include/jg.h)

    def __new__(cls, path_or_name, op, claim_set):
        path = path_or_name if isinstance(path_or_name, Path) else Path(path_or_name)
        if not isinstance(claim_set, ClaimSet):
            raise TypeError("SetRequire: the set is a ClaimSet (Validator.NewClaimSet)")
        return super().__new__(cls, (path, int(op), claim_set))

    def __repr__(self):
        return "%s(%r, <ClaimSet of %d>)" % ("InSet" if self[1] == self.IN_SET else "AnyElementIn", self[0], len(self[2]))


def InSet(path_or_name, claim_set: ClaimSet) -> SetRequire:
    """The claim is a string equal to a member of the set."""
    return SetRequire(path_or_name, SetRequire.IN_SET, claim_set)


def AnyElementIn(path_or_name, claim_set: ClaimSet) -> SetRequire:
    """The claim is an array and one of its direct elements is a string equal to a member of the set."""
    return SetRequire(path_or_name, SetRequire.ELEMENT_IN_SET, claim_set)


def _arg_requires_of(requires):
    out = []
    for r in requires:
        if isinstance(r, Require):
            out.append((list(r[0]), r[1], r[2], 0, 0))
        elif isinstance(r, ArgRequire):
            out.append((list(r[0]), r[1], r[2], r[3], r[4]))
        elif isinstance(r, SetRequire):
            out.append((list(r[0]), r[1], "", 0, r[2]._impl.token()))    # the handle travels as its token
        else:
            raise TypeError("requires: elements are built by Equals, HasWord, HasElement, Present, EqualsEach, "
                            "AtLeast, AtMost, AtLeastEach, AtMostEach, HashOfEach, IsString, InSet or AnyElementIn")
    return out


def _num_columns(nums):
    """Number columns as buffers of int64: a buffer (array('q'), a numpy int64 array) as it is, a sequence of int packed"""
    out = []
    for col in nums:
        try:
            memoryview(col)
        except TypeError:
            try:
                col = array.array("q", col)
            except OverflowError:
                raise ValueError("a number column holds a value outside int64") from None
        out.append(col)
    return out


class Validator:
    """jwt.Validator (jwt/jwt.go:20-33)."""

    def __init__(self, keyset: KeySet):
        self._ks = keyset
        self._impl = _h.Validator(keyset._impl)

    def Validate(self, token, expected: Expected = None, ctx=None):
        return tuple(self._impl.validate(token, (expected or Expected())._native()))

    def NewClaimSet(self, members, seed: int = None) -> "ClaimSet":
        """A ClaimSet of `members` (str) on this validator's key set, for InSet and
        AnyElementIn in the MatchBatchArgs family.  A NUL in a member: ValueError; a
        17th live set, or no room on the device: RuntimeError.  `seed` fixes the
        table's seed (tests); it is random per load otherwise."""
        return ClaimSet(self, members, seed)

    def ValidateBatch(self, tokens: Sequence, expected: Expected = None, ctx=None):
        """BASELINE north star: per-token result == Validate(tokens[i], expected)."""
        return [tuple(r) for r in self._impl.validate_batch(list(tokens), (expected or Expected())._native())]

    def ValidateBlob(self, blob: bytes, expected: Expected = None) -> bytes:
        """Newline-separated tokens -> one accept byte per token (throughput entry)."""
        return self._impl.validate_blob(blob, (expected or Expected())._native())

    def CheckBatch(self, tokens: Sequence, expected: Expected = None, stats: dict = None):
        """Verdict-only ValidateBatch: [err or None], err == Validate(tokens[i], expected)[1].
        The registered claims are scanned on the GPU and no claims map is built
        for a token the scan decides.  `stats` (a dict) receives {"scanned": tokens
        the device decided, "host": tokens that took the host claims path}."""
        errs, scanned, host = self._impl.check_batch(list(tokens), (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return errs

    def CheckBlob(self, blob: bytes, expected: Expected = None, stats: dict = None) -> bytes:
        """ValidateBlob's verdict-only twin (CheckBatch): newline-separated tokens ->
        one accept byte per token; `stats` as in CheckBatch."""
        ok, scanned, host = self._impl.check_blob(blob, (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return ok

    def RegisteredBatch(self, tokens: Sequence, expected: Expected = None, stats: dict = None):
        """CheckBatch plus the registered claims: [(claims or None, err or None)],
        err == Validate(tokens[i], expected)[1].  claims is go-jose's jwt.Claims of an
        accepted token: {"iss", "sub", "jti": str, "aud": [str], "exp", "nbf", "iat":
        int or None (absent or null)}.  The values come from the GPU scan with the
        verdict; no claims map is built for a token the scan decides.  `stats` as in
        CheckBatch."""
        rows, scanned, host = self._impl.registered_batch(list(tokens), (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return rows

    def RegisteredBlob(self, blob: bytes, expected: Expected = None, stats: dict = None) -> dict:
        """RegisteredBatch's throughput form: newline-separated tokens -> columns, no
        per-token Python object.  A dict of bytes: "ok" n accept bytes; "exp" / "nbf" /
        "iat" n little-endian int64 each (0 where absent); "present" n bytes with the
        date bits (bit 5 exp, 6 nbf, 7 iat); "iss" / "sub" / "jti" an (offsets, data)
        pair each, n + 1 little-endian uint32 offsets into data; "aud" (token_offsets
        [n + 1] into the elements, element_offsets into data, data).  The rows of a
        rejected token are empty.  `stats` as in CheckBatch."""
        cols, scanned, host = self._impl.registered_blob(blob, (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    def SelectBatch(self, tokens: Sequence, names: Sequence[str], expected: Expected = None, stats: dict = None):
        """RegisteredBatch plus top-level claims outside the registered seven, by name
        (scope, roles, tenant, nonce, azp, auth_time, ...): [(claims or None, values or
        None, err or None)], err == Validate(tokens[i], expected)[1] and claims as in
        RegisteredBatch.  values is a dict name -> Python value holding only the names
        the token's claims map has: exactly ValidateBatch's entries under those keys
        (case-sensitive; null is None).  The GPU scan latches where each named value
        lies; no claims map is built for a token the scan decides.  A name list the
        scan does not take (more than 8 distinct names, a name that is empty, over 64
        bytes, or not printable ASCII without quote and backslash) still answers,
        from the host path.  A name with a NUL raises ValueError.  `stats` as in
        CheckBatch.

        An element of `names` may be a Path: its value is what walking the claims map
        along it reaches -- every value on the way must be an object holding the next
        key, else the claim is absent; arrays are never descended.  The scan matches
        component j at depth j inside the objects the earlier components opened (up to
        8 distinct paths of up to 4 components; any other list still answers, from
        the host path).  In `values` the key is the element as given, str or Path.  A
        list of names alone makes exactly the call it made before."""
        names, paths = _paths_of(names)
        if paths is None:
            rows, scanned, host = self._impl.select_batch(list(tokens), names, (expected or Expected())._native())
        else:
            rows, scanned, host = self._impl.select_paths_batch(list(tokens), paths, (expected or Expected())._native())
            rows = self._keyed(rows, names)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return rows

    @staticmethod
    def _keyed(rows, names):
        """values by the path's index -> by the element of `names` as given"""
        return [(c, None if v is None else {names[k]: x for k, x in v.items()}, e) for c, v, e in rows]

    def SelectBlob(self, blob: bytes, names: Sequence[str], expected: Expected = None, stats: dict = None) -> dict:
        """SelectBatch's throughput form: newline-separated tokens -> columns.
        RegisteredBlob's dict plus "sel": one dict per name with "type" (n bytes of
        jg_sel_type: 0 absent, 1 string, 2 string with non-ASCII bytes, 3 number, 4 true,
        5 false, 6 null, 7 array, 8 object; a token the host path decided reports 1
        for any string), "num" (n little-endian float64: a number's value, else 0),
        "text_off" (n + 1 little-endian uint32) and "text": a string's UTF-8 bytes,
        an array's or object's JSON as Go's json.Marshal writes it, empty otherwise.
        The rows of a rejected token are empty.  `stats` as in CheckBatch.  `names`
        may hold Paths, as in SelectBatch: "sel" has one dict per element."""
        names, paths = _paths_of(names)
        if paths is None:
            cols, scanned, host = self._impl.select_blob(blob, names, (expected or Expected())._native())
        else:
            cols, scanned, host = self._impl.select_paths_blob(blob, paths, (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    # ---- the six entries above with an Expected per token: token i is held to
    # expected[which[i]] (its issuer, audiences, subject, ID, SigningAlgorithms, Now
    # and leeways), and its result is what the entry above returns for tokens[i]
    # alone with that Expected.  One signature submission and one GPU scan for the
    # batch, where a caller with several tenants had to make one call per tenant.
    # ValueError: len(which) != the number of tokens, an index out of range, no
    # Expected with tokens.
    @staticmethod
    def _natives(expected):
        return [e._native() for e in expected]

    def CheckBatchEach(self, tokens: Sequence, expected: Sequence[Expected], which: Sequence[int],
                       stats: dict = None):
        """CheckBatch with expected[which[i]] for tokens[i]."""
        errs, scanned, host = self._impl.check_batch_each(list(tokens), self._natives(expected), list(which))
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return errs

    def CheckBlobEach(self, blob: bytes, expected: Sequence[Expected], which, stats: dict = None) -> bytes:
        """CheckBlob with expected[which[i]] for token i; `which` is a buffer of
        uint32 (array("I"), a numpy uint32 array, ...), one per token."""
        ok, scanned, host = self._impl.check_blob_each(blob, self._natives(expected), which)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return ok

    def RegisteredBatchEach(self, tokens: Sequence, expected: Sequence[Expected], which: Sequence[int],
                            stats: dict = None):
        """RegisteredBatch with expected[which[i]] for tokens[i]."""
        rows, scanned, host = self._impl.registered_batch_each(list(tokens), self._natives(expected), list(which))
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return rows

    def RegisteredBlobEach(self, blob: bytes, expected: Sequence[Expected], which, stats: dict = None) -> dict:
        """RegisteredBlob with expected[which[i]] for token i; `which` as in CheckBlobEach."""
        cols, scanned, host = self._impl.registered_blob_each(blob, self._natives(expected), which)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    def SelectBatchEach(self, tokens: Sequence, names: Sequence[str], expected: Sequence[Expected],
                        which: Sequence[int], stats: dict = None):
        """SelectBatch with expected[which[i]] for tokens[i]; one name list for the batch."""
        names, paths = _paths_of(names)
        if paths is None:
            rows, scanned, host = self._impl.select_batch_each(list(tokens), names, self._natives(expected),
                                                               list(which))
        else:
            rows, scanned, host = self._impl.select_paths_batch_each(list(tokens), paths, self._natives(expected),
                                                                     list(which))
            rows = self._keyed(rows, names)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return rows

    def SelectBlobEach(self, blob: bytes, names: Sequence[str], expected: Sequence[Expected], which,
                       stats: dict = None) -> dict:
        """SelectBlob with expected[which[i]] for token i; `which` as in CheckBlobEach."""
        names, paths = _paths_of(names)
        if paths is None:
            cols, scanned, host = self._impl.select_blob_each(blob, names, self._natives(expected), which)
        else:
            cols, scanned, host = self._impl.select_paths_blob_each(blob, paths, self._natives(expected), which)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    # ---- yes/no questions about claims, answered by the GPU scan where the bytes are
    def MatchBatch(self, tokens: Sequence, requires: Sequence[Require], expected: Expected = None,
                   stats: dict = None):
        """CheckBatch plus requirements on claims: [(bits or None, err or None)], err ==
        Validate(tokens[i], expected)[1]; for an accepted token bit k of bits says
        whether requires[k] (Equals / HasWord / HasElement / Present, on a name or a
        Path) holds on ValidateBatch's claims map for it; a rejected token carries
        None.  A requirement never changes err.  The scan compares the values while
        it walks the payload and returns four bytes per token: no claims map, no
        text, no column.  A list the scan does not take (more than 8 distinct paths,
        a path over 4 components, a value over 64 bytes or not printable ASCII
        without quote and backslash, an empty value or one with a space for HasWord,
        an empty value for HasElement) still answers, from the host path.  More than
        16 requirements, or a NUL in a component or a value, raise ValueError.
        `stats` as in CheckBatch."""
        rows, scanned, host = self._impl.match_batch(list(tokens), _requires_of(requires),
                                                     (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return [tuple(r) for r in rows]

    def MatchBlob(self, blob: bytes, requires: Sequence[Require], expected: Expected = None,
                  stats: dict = None) -> dict:
        """MatchBatch's throughput form: newline-separated tokens -> {"ok": n accept
        bytes, "match": n little-endian uint32 masks (0 for a rejected token)}."""
        cols, scanned, host = self._impl.match_blob(blob, _requires_of(requires), (expected or Expected())._native())
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    def MatchBatchEach(self, tokens: Sequence, requires: Sequence[Require], expected: Sequence[Expected],
                       which: Sequence[int], stats: dict = None):
        """MatchBatch with expected[which[i]] for tokens[i]; one requirement list for the batch."""
        rows, scanned, host = self._impl.match_batch_each(list(tokens), _requires_of(requires),
                                                          self._natives(expected), list(which))
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return [tuple(r) for r in rows]

    def MatchBlobEach(self, blob: bytes, requires: Sequence[Require], expected: Sequence[Expected], which,
                      stats: dict = None) -> dict:
        """MatchBlob with expected[which[i]] for token i; `which` as in CheckBlobEach."""
        cols, scanned, host = self._impl.match_blob_each(blob, _requires_of(requires), self._natives(expected), which)
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols


    # ---- ... with an operand per token, and numeric tests
    def MatchBatchArgs(self, tokens: Sequence, requires: Sequence, strs: Sequence = (), nums: Sequence = (),
                       expected: Expected = None, stats: dict = None, hashes: Sequence = ()):
        """MatchBatch for the checks whose other side differs from token to token: the
        nonce of that request, auth_time under its max_age, sub against the session's
        subject.  `requires` may also hold EqualsEach(path, c) -- the claim equals
        strs[c][i] for tokens[i] --, AtLeast / AtMost(path, n) -- the claim is a
        number >= / <= n, as Go compares the claims map's float64 -- and AtLeastEach /
        AtMostEach(path, c) with nums[c][i] as n.  `strs`: columns of str, one entry
        per token; `nums`: columns of int64, each a buffer (array('q'), a numpy int64
        array) or a sequence of int.  Rows as MatchBatch's.  The scan decides a
        numeric requirement on an integer literal of at most 15 digits; a token whose
        number is written otherwise, or whose own operand the scan does not take
        (over 64 bytes, or not printable ASCII without quote and backslash) is
        answered from the host path, as is every token of a list over the scan's caps
        (MatchBatch's, or more than 4 columns of a kind).  A column whose length is
        not len(tokens), a column index without a column, more than 16 requirements,
        a NUL in an operand: ValueError.

        `hashes`: hash columns, one entry of bytes / str / None per token, for
        HashOfEach(path, c): the claim equals base64url(SHA-2(hashes[c][i])[:half])
        with the SHA-2 of tokens[i]'s alg -- at_hash against the access token, c_hash
        against the authorization code -- hashed and encoded on the device in front of
        the scan.  With IsString(path) the pair maps to Go's (verified, err) of
        IDToken.VerifyAccessToken / VerifyAuthorizationCode: verified = IsString &
        HashOfEach; err != nil exactly when IsString holds, HashOfEach does not and
        the alg is not EdDSA.  A value over 8192 bytes is hashed on the host path.
        At most 2 hash columns, and 4 string and hash columns together, are scanned.
        A hash column whose length is not len(tokens), or a hash column index without
        a column: ValueError."""
        rows, scanned, host = self._impl.match_batch_args(list(tokens), _arg_requires_of(requires),
                                                          [list(c) for c in strs], _num_columns(nums),
                                                          (expected or Expected())._native(), [list(c) for c in hashes])
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return [tuple(r) for r in rows]

    def MatchBlobArgs(self, blob: bytes, requires: Sequence, strs: Sequence = (), nums: Sequence = (),
                      expected: Expected = None, stats: dict = None, hashes: Sequence = ()) -> dict:
        """MatchBatchArgs' throughput form: newline-separated tokens and, per string
        column, newline-separated operands (bytes; an empty line is the operand "")
        -> MatchBlob's columns.  A hash column is newline-separated values too; an
        empty line means "no value"."""
        cols, scanned, host = self._impl.match_blob_args(blob, _arg_requires_of(requires), [bytes(c) for c in strs],
                                                         _num_columns(nums), (expected or Expected())._native(),
                                                         [bytes(c) for c in hashes])
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols

    def MatchBatchArgsEach(self, tokens: Sequence, requires: Sequence, expected: Sequence[Expected],
                           which: Sequence[int], strs: Sequence = (), nums: Sequence = (), stats: dict = None,
                           hashes: Sequence = ()):
        """MatchBatchArgs with expected[which[i]] for tokens[i]."""
        rows, scanned, host = self._impl.match_batch_args_each(list(tokens), _arg_requires_of(requires),
                                                               [list(c) for c in strs], _num_columns(nums),
                                                               self._natives(expected), list(which),
                                                               [list(c) for c in hashes])
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return [tuple(r) for r in rows]

    def MatchBlobArgsEach(self, blob: bytes, requires: Sequence, expected: Sequence[Expected], which,
                          strs: Sequence = (), nums: Sequence = (), stats: dict = None, hashes: Sequence = ()) -> dict:
        """MatchBlobArgs with expected[which[i]] for token i; `which` as in CheckBlobEach."""
        cols, scanned, host = self._impl.match_blob_args_each(blob, _arg_requires_of(requires),
                                                              [bytes(c) for c in strs], _num_columns(nums),
                                                              self._natives(expected), which, [bytes(c) for c in hashes])
        if stats is not None:
            stats.update(scanned=scanned, host=host)
        return cols


def NewValidator(keyset: Optional[KeySet]):
    if keyset is None:
        return None, "keySet must not be nil"
    return Validator(keyset), None


__all__ = ["RS256", "RS384", "RS512", "ES256", "ES384", "ES512", "PS256", "PS384", "PS512", "EdDSA",
           "DefaultLeewaySeconds", "PublicKey", "SupportedSigningAlgorithm", "ParsePublicKeyPEM", "KeySet",
           "NewStaticKeySet", "NewJSONWebKeySet", "NewOIDCDiscoveryKeySet", "Expected", "Path", "Validator",
           "NewValidator", "ClaimSet", "SetRequire", "InSet", "AnyElementIn", "Require", "Equals", "HasWord", "HasElement", "Present", "ArgRequire", "EqualsEach",
           "AtLeast", "AtMost", "AtLeastEach", "AtMostEach", "HashOfEach", "IsString"]
