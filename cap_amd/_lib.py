"""ctypes binding of the C ABI in include/jg.h (libcapjwt.so).

This is plumbing for tests / bench / the Python mirror of cap's jwt package;
the product is the shared library.  There is deliberately no CPU fallback:
if libcapjwt.so is missing or no HIP device is present, every entry point
raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CAPJWT_LIB") or os.path.join(HERE, "libcapjwt.so")

# jwt/algs.go:12-21
ALG_IDS = {"RS256": 1, "RS384": 2, "RS512": 3, "PS256": 4, "PS384": 5, "PS512": 6,
           "ES256": 7, "ES384": 8, "ES512": 9, "EdDSA": 10}
KEY_RSA, KEY_EC, KEY_ED25519 = 1, 2, 3
CURVE_IDS = {"P-256": 1, "P-384": 2, "P-521": 3}
# jg_debug_table_read: the fixed-base tables (JG_TABLE_*), and what Context.table_read pre-fills its buffer with
TABLE_P256_G, TABLE_P384_G, TABLE_P521_G, TABLE_ED25519_B = -1, -2, -3, -4
TABLE_READ_FILL = 0xA5A5A5A5

# every symbol include/jg.h declares
EXPORTS = ["jg_create", "jg_destroy", "jg_keys_load", "jg_verify_batch", "jg_last_error",
           "jg_host_alloc", "jg_host_free", "jg_batch_stage", "jg_batch_run", "jg_batch_enqueue", "jg_batch_sync",
           "jg_batch_free", "jg_batch_kernel_times", "jg_batch_exceptions", "jg_hash_batch", "jg_version",
           "jg_submit", "jg_wait", "jg_set_chunk", "jg_set_zero_copy", "jg_set_table_budget", "jg_keys_wait_tables",
           "jg_keys_table_widths", "jg_debug_fail_alloc", "jg_debug_table_digest", "jg_debug_table_read",
           "jg_debug_max_upgrades", "jg_debug_lifetime_check", "jg_debug_fail_verify", "jg_debug_tables_built",
           "jg_debug_small_path", "jg_claims_scan", "jg_claims_extract", "jg_claims_select", "jg_claims_each",
           "jg_claims_paths", "jg_claims_match", "jg_claims_match_args", "jg_claims_match_hash",
           "jg_set_load", "jg_set_free", "jg_set_info", "jg_debug_set_read", "jg_claims_match_set", "jg_set_add"]


class JgKey(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("curve", ctypes.c_int32),
                ("n", ctypes.c_void_p), ("n_len", ctypes.c_int32), ("e", ctypes.c_uint64),
                ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("coord_len", ctypes.c_int32)]


class JgTok(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("sig_in_len", ctypes.c_uint32), ("sig_rel_off", ctypes.c_uint32),
                ("sig_b64_len", ctypes.c_uint32), ("key_idx", ctypes.c_uint16), ("alg", ctypes.c_uint8),
                ("flags", ctypes.c_uint8)]


assert ctypes.sizeof(JgTok) == 24

MAX_AUD = 16                       # JG_MAX_AUD
MAX_PROFILES, PROFILE_POOL_BYTES = 64, 8192      # JG_MAX_PROFILES, JG_PROFILE_POOL_BYTES
# jg_claim_code
CL_OK, CL_NO_TIME, CL_ISS, CL_SUB, CL_JTI, CL_AUD, CL_NBF, CL_EXP, CL_IAT, CL_HOST = range(10)
# the string Validator.Validate gives for each code (jwt/jwt.go:117-199)
CLAIM_ERRORS = {
    CL_OK: None,
    CL_NO_TIME: "no issued at (iat), not before (nbf), or expiration time (exp) claims in token",
    CL_ISS: "invalid issuer (iss) claim",
    CL_SUB: "invalid subject (sub) claim",
    CL_JTI: "invalid ID (jti) claim",
    CL_AUD: "invalid audience (aud) claim: audience claim does not match any expected audience",
    CL_NBF: "invalid not before (nbf) claim: token not yet valid",
    CL_EXP: "invalid expiration time (exp) claim: token is expired",
    CL_IAT: "invalid issued at (iat) claim: token issued in the future",
}


class JgCJob(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class JgExpect(ctypes.Structure):
    _fields_ = [("strs", ctypes.c_void_p), ("iss_len", ctypes.c_uint32), ("sub_len", ctypes.c_uint32),
                ("jti_len", ctypes.c_uint32), ("naud", ctypes.c_uint32), ("aud_len", ctypes.c_uint32 * MAX_AUD),
                ("now_sec", ctypes.c_int64), ("now_nsec", ctypes.c_uint32), ("pad_", ctypes.c_uint32),
                ("skew_ns", ctypes.c_int64), ("exp_leeway_s", ctypes.c_int64), ("nbf_leeway_s", ctypes.c_int64)]


assert ctypes.sizeof(JgCJob) == 16


class JgClaims(ctypes.Structure):
    """jg_claims: the registered claims jg_claims_extract read from one payload"""
    _fields_ = [("exp", ctypes.c_int64), ("nbf", ctypes.c_int64), ("iat", ctypes.c_int64),
                ("iss_off", ctypes.c_uint32), ("iss_len", ctypes.c_uint32),
                ("sub_off", ctypes.c_uint32), ("sub_len", ctypes.c_uint32),
                ("jti_off", ctypes.c_uint32), ("jti_len", ctypes.c_uint32),
                ("aud_off", ctypes.c_uint32), ("aud_len", ctypes.c_uint32),
                ("aud_n", ctypes.c_uint32), ("present", ctypes.c_uint32)]


assert ctypes.sizeof(JgClaims) == 64
# bit f of jg_claims.present (F_ISS .. F_IAT of kernels/claims.hpp)
F_ISS, F_SUB, F_JTI, F_AUD, F_EXP, F_NBF, F_IAT = range(1, 8)

MAX_SELECT, SELECT_NAME_MAX = 8, 64          # JG_MAX_SELECT, JG_SELECT_NAME_MAX
# jg_sel_type
(SEL_ABSENT, SEL_STRING, SEL_STRING_RAW, SEL_NUMBER, SEL_TRUE, SEL_FALSE, SEL_NULL, SEL_ARRAY,
 SEL_OBJECT) = range(9)


class JgSelect(ctypes.Structure):
    """jg_select: the caller's claim names, back to back in `names`"""
    _fields_ = [("names", ctypes.c_void_p), ("n", ctypes.c_uint32), ("name_len", ctypes.c_uint32 * MAX_SELECT)]


class JgSelected(ctypes.Structure):
    """jg_selected: where the named top-level members of one payload lie"""
    _fields_ = [("off", ctypes.c_uint32 * MAX_SELECT), ("len", ctypes.c_uint32 * MAX_SELECT),
                ("type", ctypes.c_uint8 * MAX_SELECT), ("pad_", ctypes.c_uint8 * 8)]


assert ctypes.sizeof(JgSelected) == 80

MAX_PATHS, PATH_MAX_COMP = 8, 4              # JG_MAX_PATHS, JG_PATH_MAX_COMP


class JgPaths(ctypes.Structure):
    """jg_paths: the caller's claim paths, their components back to back in `names`"""
    _fields_ = [("names", ctypes.c_void_p), ("n", ctypes.c_uint32), ("ncomp", ctypes.c_uint32 * MAX_PATHS),
                ("comp_len", (ctypes.c_uint32 * PATH_MAX_COMP) * MAX_PATHS)]


MAX_PRED, PRED_VALUE_MAX = 16, 64            # JG_MAX_PRED, JG_PRED_VALUE_MAX
# jg_pred_op
PRED_EQUALS, PRED_HAS_WORD, PRED_HAS_ELEMENT, PRED_PRESENT = 1, 2, 3, 4
# ... and those only jg_claims_match_args takes: the value is a column index (one byte) or an int64 bound
PRED_EQUALS_ARG, PRED_NUM_GE, PRED_NUM_LE, PRED_NUM_GE_ARG, PRED_NUM_LE_ARG = 5, 6, 7, 8, 9
MAX_ARGS = 4                                 # JG_MAX_ARGS
# ... and those only jg_claims_match_hash takes: the value is a hash column index (one byte), or nothing
PRED_EQUALS_HASH, PRED_IS_STRING = 10, 11
MAX_HASH_ARGS, HASH_SRC_MAX = 2, 8192        # JG_MAX_HASH_ARGS, JG_HASH_SRC_MAX
SHA256, SHA384, SHA512 = 1, 2, 3             # jg_hash_fam; 0 in a jg_hsrc: the job has no value


class JgPreds(ctypes.Structure):
    """jg_preds: the caller's predicates, their values back to back in `values`"""
    _fields_ = [("values", ctypes.c_void_p), ("n", ctypes.c_uint32), ("path", ctypes.c_uint8 * MAX_PRED),
                ("op", ctypes.c_uint8 * MAX_PRED), ("value_len", ctypes.c_uint32 * MAX_PRED)]


class JgSArg(ctypes.Structure):
    """jg_sarg: one string operand, a span of jg_args.bytes"""
    _fields_ = [("off", ctypes.c_uint32), ("len", ctypes.c_uint32)]


class JgArgs(ctypes.Structure):
    """jg_args: the per-job operands of jg_claims_match_args"""
    _fields_ = [("bytes", ctypes.c_void_p), ("bytes_len", ctypes.c_size_t), ("str", ctypes.c_void_p),
                ("num", ctypes.c_void_p), ("nstr", ctypes.c_uint32), ("nnum", ctypes.c_uint32)]


assert ctypes.sizeof(JgSArg) == 8


class JgHSrc(ctypes.Structure):
    """jg_hsrc: one value to hash, a span of jg_hargs.bytes and its family"""
    _fields_ = [("off", ctypes.c_uint32), ("len", ctypes.c_uint32), ("fam", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3)]


class JgHArgs(ctypes.Structure):
    """jg_hargs: the per-job hash sources of jg_claims_match_hash"""
    _fields_ = [("bytes", ctypes.c_void_p), ("bytes_len", ctypes.c_size_t), ("src", ctypes.c_void_p),
                ("nhash", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


assert ctypes.sizeof(JgHSrc) == 12 and ctypes.sizeof(JgHArgs) == 32


# ... and those only jg_claims_match_set takes: the value is a set index of the call (one byte)
PRED_IN_SET, PRED_ELEMENT_IN_SET = 12, 13
MAX_SETS, MAX_LOADED_SETS, SET_MEMBER_MAX = 4, 16, 255   # JG_MAX_SETS, JG_MAX_LOADED_SETS, JG_SET_MEMBER_MAX


class JgSetInfo(ctypes.Structure):
    """jg_setinfo: what jg_set_info reports of a loaded set"""
    _fields_ = [("n", ctypes.c_uint32), ("nslots", ctypes.c_uint32), ("maxprobe", ctypes.c_uint32),
                ("seed", ctypes.c_uint32), ("pool_bytes", ctypes.c_uint64), ("generation", ctypes.c_uint64)]


class JgSetArgs(ctypes.Structure):
    """jg_setargs: the loaded sets a jg_claims_match_set call names"""
    _fields_ = [("nsets", ctypes.c_uint32), ("id", ctypes.c_uint32 * MAX_SETS)]


assert ctypes.sizeof(JgSetInfo) == 32 and ctypes.sizeof(JgSetArgs) == 20


def _jg_setargs(ids, nsets=None):
    """Set ids -> JgSetArgs (ids past what the struct holds are dropped: the call is refused on its count)"""
    g = JgSetArgs()
    g.nsets = len(ids) if nsets is None else nsets
    for k, x in enumerate(list(ids)[:MAX_SETS]):
        g.id[k] = x
    return g


def pack_hargs(cols=(), lead=0):
    """Hash columns -> the dict Context.claims_match_hash takes.  `cols`: hash
    columns, each one (value bytes, fam) per job, or None for "no value" (fam 0,
    an empty span).  The values are packed job-major, back to back after `lead`
    filler bytes, so the last one ends at the last byte.  {"bytes", "src": a row of
    (off, len, fam) per job, "nhash"}: a test may edit any of it."""
    n = len(cols[0]) if cols else 0
    blob, src = bytearray(b"#" * lead), []
    for i in range(n):
        row = []
        for col in cols:
            v, fam = col[i] if col[i] is not None else (b"", 0)
            row.append((len(blob), len(v), fam))
            blob += bytes(v)
        src.append(row)
    return {"bytes": bytes(blob), "src": src, "nhash": len(cols)}


def _jg_hargs(a, null=()):
    """pack_hargs' dict -> (JgHArgs, the buffers to keep alive)"""
    blob = a["bytes"]
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    flat = [x for row in a["src"] for x in row]
    sp = (JgHSrc * max(1, len(flat)))()
    for t, (off, ln, fam) in zip(sp, flat):
        t.off, t.len, t.fam = off, ln, fam
    g = JgHArgs()
    g.bytes = None if "hbytes" in null else ctypes.cast(keep, ctypes.c_void_p)
    g.bytes_len = a.get("bytes_len", len(blob))
    g.src = None if "hsrc" in null else ctypes.cast(sp, ctypes.c_void_p)
    g.nhash = a["nhash"]
    return g, (keep, sp)


def pack_args(strs=(), nums=(), lead=0):
    """Operand columns -> the dict Context.claims_match_args takes.  `strs`: string
    columns, each one bytes per job; `nums`: int64 columns, each one int per job.
    The operands are packed job-major, back to back after `lead` filler bytes, so
    the last one ends at the last byte.  {"bytes", "spans": a row of (off, len) per
    job, "nums": a row of ints per job, "nstr", "nnum"}: a test may edit any of it."""
    n = len(strs[0]) if strs else len(nums[0]) if nums else 0
    blob, spans = bytearray(b"#" * lead), []
    for i in range(n):
        row = []
        for col in strs:
            v = bytes(col[i])
            row.append((len(blob), len(v)))
            blob += v
        spans.append(row)
    return {"bytes": bytes(blob), "spans": spans, "nums": [[int(col[i]) for col in nums] for i in range(n)],
            "nstr": len(strs), "nnum": len(nums)}


def _jg_args(a, null=()):
    """pack_args' dict -> (JgArgs, the buffers to keep alive)"""
    blob = a["bytes"]
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    flat = [x for row in a["spans"] for x in row]
    sp = (JgSArg * max(1, len(flat)))()
    for t, (off, ln) in zip(sp, flat):
        t.off, t.len = off, ln
    fn = [x for row in a["nums"] for x in row]
    nm = (ctypes.c_int64 * max(1, len(fn)))(*fn)
    g = JgArgs()
    g.bytes = None if "bytes" in null else ctypes.cast(keep, ctypes.c_void_p)
    g.bytes_len = a.get("bytes_len", len(blob))
    g.str = None if "str" in null else ctypes.cast(sp, ctypes.c_void_p)
    g.num = None if "num" in null else ctypes.cast(nm, ctypes.c_void_p)
    g.nstr, g.nnum = a["nstr"], a["nnum"]
    return g, (keep, sp, nm)


def _cjobs(rows):
    """(off, len, flags) rows -> a JgCJob array (of one unused job for no rows)"""
    rows = list(rows)
    cj = (JgCJob * max(1, len(rows)))()
    for j, (off, ln, flags) in zip(cj, rows):
        j.off, j.len, j.flags = off, ln, flags
    return cj


def _jg_expect(d, e=None):
    """An Expected dict (Context.claims_scan) -> (JgExpect, the buffer its strs points into:
    to be kept alive).  `e`: the JgExpect to fill."""
    e = JgExpect() if e is None else e
    auds = [bytes(a) for a in d.get("audiences", [])]
    strs = [bytes(d.get(k, b"")) for k in ("issuer", "subject", "id")]
    blob = b"".join(strs + auds)
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    e.strs = ctypes.cast(keep, ctypes.c_void_p)
    e.iss_len, e.sub_len, e.jti_len = (len(x) for x in strs)
    e.naud = len(auds)
    for k, a in enumerate(auds[:MAX_AUD]):
        e.aud_len[k] = len(a)
    e.now_sec, e.now_nsec = int(d["now_sec"]), int(d["now_nsec"])
    e.skew_ns = int(d["skew_ns"])
    e.exp_leeway_s, e.nbf_leeway_s = int(d["exp_leeway_s"]), int(d["nbf_leeway_s"])
    return e, keep


def _jg_expects(ds):
    """A list of Expected dicts -> (JgExpect array, the buffers to keep alive)"""
    es = (JgExpect * max(1, len(ds)))()
    return es, [_jg_expect(d, e)[1] for e, d in zip(es, ds)]


def _jg_select(names):
    """Claim names -> (JgSelect, the buffer to keep alive)"""
    names = [bytes(x) for x in names]
    blob = b"".join(names)
    sel = JgSelect()
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    sel.names = ctypes.cast(keep, ctypes.c_void_p)
    sel.n = len(names)
    for k, x in enumerate(names[:MAX_SELECT]):
        sel.name_len[k] = len(x)
    return sel, keep


def _jg_paths(paths):
    """Claim paths, each a sequence of components -> (JgPaths, the buffer to keep alive)"""
    paths = [[bytes(c) for c in path] for path in paths]
    ps = JgPaths()
    ps.n = len(paths)
    blob = b""
    for k, path in enumerate(paths[:MAX_PATHS]):
        ps.ncomp[k] = len(path)
        for d, c in enumerate(path[:PATH_MAX_COMP]):        # past what the struct holds the path is refused on its count
            ps.comp_len[k][d] = len(c)
            blob += c
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    ps.names = ctypes.cast(keep, ctypes.c_void_p)
    return ps, keep


def _jg_preds(preds):
    """Predicates, each (path index, op, value bytes) -> (JgPreds, the buffer to keep alive)"""
    preds = [(int(p), int(op), bytes(v)) for p, op, v in preds]
    ps = JgPreds()
    ps.n = len(preds)
    blob = b""
    for k, (path, op, value) in enumerate(preds[:MAX_PRED]):   # past what the struct holds the list is refused on its count
        ps.path[k], ps.op[k], ps.value_len[k] = path, op, len(value)
        blob += value
    keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
    ps.values = ctypes.cast(keep, ctypes.c_void_p)
    return ps, keep


def _poisoned(ctype, n):
    """An output array of max(1, n) records, every byte 0xee"""
    buf = (ctype * max(1, n))()
    ctypes.memset(buf, 0xee, ctypes.sizeof(buf))
    return buf


def _records(ctype, buf, n):
    """The first n records of an output array, copied out"""
    return (ctype * n).from_buffer_copy(bytes(buf)[:ctypes.sizeof(ctype) * n])



_lib = None


class JgError(RuntimeError):
    pass


def lib():
    """Load libcapjwt.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JgError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.jg_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        L.jg_create.restype = vp
        L.jg_destroy.argtypes = [vp]
        L.jg_keys_load.argtypes = [vp, ctypes.POINTER(JgKey), ctypes.c_int]
        L.jg_verify_batch.argtypes = [vp, vp, sz, ctypes.POINTER(JgTok), sz, vp]
        L.jg_last_error.argtypes = [vp]
        L.jg_last_error.restype = ctypes.c_char_p
        L.jg_host_alloc.argtypes = [sz]
        L.jg_host_alloc.restype = vp
        L.jg_host_free.argtypes = [vp]
        L.jg_batch_stage.argtypes = [vp, ctypes.c_int, vp, sz, ctypes.POINTER(JgTok), sz, ctypes.POINTER(vp)]
        L.jg_batch_run.argtypes = [vp, vp, vp]
        L.jg_batch_enqueue.argtypes = [vp, vp, vp]
        L.jg_batch_sync.argtypes = [vp, vp]
        L.jg_batch_free.argtypes = [vp, vp]
        L.jg_batch_kernel_times.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float),
                                            ctypes.c_int]
        L.jg_batch_exceptions.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
        L.jg_submit.argtypes = [vp, vp, sz, ctypes.POINTER(JgTok), sz, vp, ctypes.POINTER(vp)]
        L.jg_wait.argtypes = [vp, vp]
        L.jg_set_chunk.argtypes = [vp, sz]
        L.jg_set_zero_copy.argtypes = [vp, ctypes.c_int, sz]
        L.jg_set_table_budget.argtypes = [vp, ctypes.c_uint64]
        L.jg_hash_batch.argtypes = [vp, vp, sz, vp, sz, vp]
        L.jg_claims_scan.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect), vp]
        L.jg_claims_extract.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect), vp, vp]
        L.jg_claims_select.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                       ctypes.POINTER(JgSelect), vp, vp, vp]
        L.jg_claims_each.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                     ctypes.c_uint32, ctypes.POINTER(JgSelect), vp, vp, vp]
        L.jg_claims_paths.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                      ctypes.c_uint32, ctypes.POINTER(JgPaths), vp, vp, vp]
        L.jg_claims_match.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                      ctypes.c_uint32, ctypes.POINTER(JgPaths), ctypes.POINTER(JgPreds), vp, vp]
        L.jg_claims_match_args.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                           ctypes.c_uint32, ctypes.POINTER(JgPaths), ctypes.POINTER(JgPreds),
                                           ctypes.POINTER(JgArgs), vp, vp]
        L.jg_claims_match_hash.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                           ctypes.c_uint32, ctypes.POINTER(JgPaths), ctypes.POINTER(JgPreds),
                                           ctypes.POINTER(JgArgs), ctypes.POINTER(JgHArgs), vp, vp]
        L.jg_claims_match_set.argtypes = [vp, vp, sz, ctypes.POINTER(JgCJob), sz, ctypes.POINTER(JgExpect),
                                          ctypes.c_uint32, ctypes.POINTER(JgPaths), ctypes.POINTER(JgPreds),
                                          ctypes.POINTER(JgArgs), ctypes.POINTER(JgHArgs), ctypes.POINTER(JgSetArgs),
                                          vp, vp]
        L.jg_set_load.argtypes = [vp, ctypes.c_uint32, vp, sz, vp, sz, ctypes.c_uint32]
        L.jg_set_add.argtypes = [vp, ctypes.c_uint32, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint32)]
        L.jg_set_free.argtypes = [vp, ctypes.c_uint32]
        L.jg_set_info.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(JgSetInfo)]
        L.jg_debug_set_read.argtypes = [vp, ctypes.c_uint32, vp, sz, vp, sz]
        L.jg_keys_wait_tables.argtypes = [vp]
        L.jg_keys_table_widths.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        L.jg_debug_fail_alloc.argtypes = [vp, ctypes.c_int]
        L.jg_debug_max_upgrades.argtypes = [vp, ctypes.c_int]
        L.jg_debug_fail_verify.argtypes = [vp, ctypes.c_int]
        L.jg_debug_lifetime_check.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_uint64)]
        L.jg_debug_table_digest.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.jg_debug_table_read.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, vp, sz] + \
            [ctypes.POINTER(ctypes.c_int)] * 4
        L.jg_debug_tables_built.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
        L.jg_debug_small_path.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.jg_version.restype = ctypes.c_char_p
        _lib = L
    return _lib


def lifetime_check(enable=-1):
    """jg_debug_lifetime_check: 1 / 0 turns the key-memory lifetime check on /
    off (-1 leaves it); returns (violations, events checked) so far."""
    bad, chk = ctypes.c_uint64(), ctypes.c_uint64()
    lib().jg_debug_lifetime_check(int(enable), ctypes.byref(bad), ctypes.byref(chk))
    return bad.value, chk.value


class Key:
    """A public key handed to jg_keys_load (bytes are big-endian; Ed25519: raw 32 bytes)."""

    def __init__(self, kind, n=b"", e=0, curve=0, x=b"", y=b""):
        self.kind, self.n, self.e, self.curve, self.x, self.y = kind, n, e, curve, x, y

    @staticmethod
    def rsa(n: bytes, e: int):
        return Key(KEY_RSA, n=n, e=e)

    @staticmethod
    def ec(curve: str, x: bytes, y: bytes):
        return Key(KEY_EC, curve=CURVE_IDS[curve], x=x, y=y)

    @staticmethod
    def ed25519(pub: bytes):
        return Key(KEY_ED25519, x=pub)


class Arena:
    """Packed job list: signing inputs and base64url signatures in one buffer."""

    def __init__(self):
        self.buf = bytearray()
        self.toks = []

    def add(self, signing_input: bytes, sig_b64: bytes, alg: str, key_idx: int):
        sig_b64 = sig_b64.rstrip(b"=")
        off = len(self.buf)
        self.buf += signing_input + b"." + sig_b64
        self.toks.append((off, len(signing_input), len(signing_input) + 1, len(sig_b64), key_idx,
                          ALG_IDS.get(alg, 0)))
        return len(self.toks) - 1

    def tok_array(self):
        arr = (JgTok * max(1, len(self.toks)))()
        for i, t in enumerate(self.toks):
            arr[i].off, arr[i].sig_in_len, arr[i].sig_rel_off, arr[i].sig_b64_len, arr[i].key_idx, arr[i].alg = t
        return arr


class Context:
    """Owns a jg_ctx on the given HIP devices."""

    def __init__(self, devices=None):
        L = lib()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            self.h = L.jg_create(arr, len(devices))
        else:
            self.h = L.jg_create(None, 0)
        if not self.h:
            raise JgError("jg_create failed: " + (L.jg_last_error(None) or b"").decode())
        self._keep = []

    def close(self):
        if self.h:
            lib().jg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self):
        return (lib().jg_last_error(self.h) or b"").decode()

    def load_keys(self, keys, wait_tables=True):
        """jg_keys_load; with wait_tables (default) also jg_keys_wait_tables, so
        every key runs at its budgeted comb width when this returns."""
        arr = (JgKey * max(1, len(keys)))()
        keep = []
        for i, k in enumerate(keys):
            arr[i].kind = k.kind
            arr[i].curve = k.curve
            for fld in ("n", "x", "y"):
                b = getattr(k, fld)
                if b:
                    cb = ctypes.create_string_buffer(bytes(b), len(b))
                    keep.append(cb)
                    setattr(arr[i], fld, ctypes.cast(cb, ctypes.c_void_p))
            arr[i].n_len = len(k.n)
            arr[i].e = k.e
            arr[i].coord_len = len(k.x) if k.kind != KEY_RSA else 0
        rc = lib().jg_keys_load(self.h, arr, len(keys))
        if rc != 0:
            raise JgError(f"jg_keys_load rc={rc}: {self.error()}")
        if wait_tables:
            self.wait_tables()

    def wait_tables(self):
        """jg_keys_wait_tables: True when every table reached its budgeted width."""
        rc = lib().jg_keys_wait_tables(self.h)
        if rc < 0:
            raise JgError(f"jg_keys_wait_tables rc={rc}")
        return rc == 0

    def table_widths(self):
        """jg_keys_table_widths: comb width per loaded key (0 = none)."""
        n = lib().jg_keys_table_widths(self.h, None, 0)
        arr = (ctypes.c_int * max(1, n))()
        lib().jg_keys_table_widths(self.h, arr, n)
        return list(arr[:n])

    def table_digest(self, key):
        """jg_debug_table_digest: 64-bit digest of key `key`'s comb table (0 = none)."""
        v = ctypes.c_uint64()
        if lib().jg_debug_table_digest(self.h, int(key), ctypes.byref(v)) != 0:
            raise JgError(f"jg_debug_table_digest: {self.error()}")
        return v.value

    def table_read(self, key, first_entry=0, n_entries=0, out_words=None):
        """jg_debug_table_read: raw words of n_entries comb-table entries of key
        `key` (or of a fixed-base table: TABLE_P256_G .. TABLE_ED25519_B) from
        entry first_entry on.  Returns (words, cls, width, nwin, stride_words);
        n_entries = 0 reads the geometry alone.  out_words: the buffer's size
        in words when it is to differ from what the entries need.  Raises
        JgError where the hook refuses; the error's `words` holds the buffer,
        which the hook then left untouched."""
        geo = [ctypes.c_int(0) for _ in range(4)]
        refs = [ctypes.byref(g) for g in geo]
        L = lib()
        if out_words is None:
            if L.jg_debug_table_read(self.h, int(key), 0, 0, None, 0, *refs) != 0:
                raise JgError(f"jg_debug_table_read: {self.error()}")
            out_words = int(n_entries) * geo[3].value
        buf = (ctypes.c_uint32 * max(1, int(out_words)))(*([TABLE_READ_FILL] * max(1, int(out_words))))
        rc = L.jg_debug_table_read(self.h, int(key), int(first_entry), int(n_entries), buf, int(out_words), *refs)
        if rc != 0:
            e = JgError(f"jg_debug_table_read rc={rc}: {self.error()}")
            e.words = list(buf)
            raise e
        return (list(buf[:int(n_entries) * geo[3].value]),) + tuple(g.value for g in geo)

    def tables_built(self):
        """jg_debug_tables_built: comb tables this context has built (cache reuses excluded)."""
        v = ctypes.c_uint64()
        if lib().jg_debug_tables_built(self.h, ctypes.byref(v)) != 0:
            raise JgError(f"jg_debug_tables_built: {self.error()}")
        return v.value

    def debug_max_upgrades(self, n):
        """jg_debug_max_upgrades: the background upgrader widens at most n more tables (-1 = no limit)."""
        if lib().jg_debug_max_upgrades(self.h, int(n)) != 0:
            raise JgError("jg_debug_max_upgrades failed")

    def debug_small_path(self, enable=None):
        """jg_debug_small_path: small submissions of the one-launch classes (ECDSA on
        P-256 / P-384 / P-521, EdDSA, RSA-2048 PKCS#1 v1.5) as one launch per (class,
        key-table width) (True, the default) or through the batch chain (False; None
        leaves it); returns the number of such launches enqueued so far -- the counter
        counts launches, not tokens.  Verdicts are identical."""
        v = ctypes.c_uint64()
        if lib().jg_debug_small_path(self.h, -1 if enable is None else (1 if enable else 0), ctypes.byref(v)) != 0:
            raise JgError("jg_debug_small_path failed")
        return v.value

    def debug_fail_alloc(self, n):
        """jg_debug_fail_alloc: the n-th device allocation of later key loads fails (0 = off)."""
        if lib().jg_debug_fail_alloc(self.h, int(n)) != 0:
            raise JgError("jg_debug_fail_alloc failed")

    def debug_fail_verify(self, n):
        """jg_debug_fail_verify: the n-th later submission fails as a device fault and the
        context stays unusable (0 = off)."""
        if lib().jg_debug_fail_verify(self.h, int(n)) != 0:
            raise JgError("jg_debug_fail_verify failed")

    def verify(self, arena: Arena):
        n = len(arena.toks)
        out = (ctypes.c_uint8 * max(1, n))()
        buf = bytes(arena.buf) or b"\0"
        rc = lib().jg_verify_batch(self.h, buf, len(arena.buf), arena.tok_array(), n, out)
        if rc != 0:
            raise JgError(f"jg_verify_batch rc={rc}: {self.error()}")
        return bytes(out[:n])

    def _claims_call(self, entry, arena_bytes, cj, n, *args):
        buf = bytes(arena_bytes) or b"\0"
        rc = getattr(lib(), entry)(self.h, buf, len(arena_bytes), cj, n, *args)
        if rc != 0:
            raise JgError(f"{entry} rc={rc}: {self.error()}")

    def claims_scan(self, arena_bytes, spans, expect, flags=0):
        """jg_claims_scan: one jg_claim_code byte per (off, len) span of base64url
        payload segment in `arena_bytes`.  `expect`: a dict with issuer, subject,
        id (bytes), audiences (list of bytes), now_sec, now_nsec, skew_ns,
        exp_leeway_s, nbf_leeway_s -- already resolved (see include/jg.h)."""
        n = len(spans)
        e, _keep = _jg_expect(expect)
        out = _poisoned(ctypes.c_char, n)
        self._claims_call("jg_claims_scan", arena_bytes, _cjobs((o, ln, flags) for o, ln in spans), n,
                          ctypes.byref(e), out)
        return out.raw[:n]

    def claims_extract(self, arena_bytes, spans, expect, flags=0):
        """jg_claims_extract: claims_scan's codes and, per span, the jg_claims
        record of the registered claims -> (codes: bytes, vals: JgClaims array).
        Both outputs are poisoned with 0xee before the call."""
        n = len(spans)
        e, _keep = _jg_expect(expect)
        out, vals = _poisoned(ctypes.c_char, n), _poisoned(JgClaims, n)
        self._claims_call("jg_claims_extract", arena_bytes, _cjobs((o, ln, flags) for o, ln in spans), n,
                          ctypes.byref(e), out, ctypes.cast(vals, ctypes.c_void_p))
        return out.raw[:n], _records(JgClaims, vals, n)

    def claims_select(self, arena_bytes, spans, expect, names, flags=0):
        """jg_claims_select: claims_extract's codes and records and, per span, the
        jg_selected record of the top-level members `names` (a list of bytes) name
        -> (codes: bytes, vals: JgClaims array, sels: JgSelected array).  All three
        outputs are poisoned with 0xee before the call."""
        n = len(spans)
        e, _keep = _jg_expect(expect)
        sel, _nkeep = _jg_select(names)
        out, vals, sels = _poisoned(ctypes.c_char, n), _poisoned(JgClaims, n), _poisoned(JgSelected, n)
        self._claims_call("jg_claims_select", arena_bytes, _cjobs((o, ln, flags) for o, ln in spans), n,
                          ctypes.byref(e), ctypes.byref(sel), out, ctypes.cast(vals, ctypes.c_void_p),
                          ctypes.cast(sels, ctypes.c_void_p))
        return out.raw[:n], _records(JgClaims, vals, n), _records(JgSelected, sels, n)

    def claims_each(self, arena_bytes, jobs, expects, mode="scan", names=None, nexpect=None):
        """jg_claims_each: the three scans with a profile per job.  `jobs`: (off,
        len, profile) triples; `expects`: a list of dicts as claims_scan takes one;
        mode "scan" -> codes, "extract" -> (codes, vals), "select" (with `names`)
        -> (codes, vals, sels), as claims_scan / claims_extract / claims_select
        return them.  The outputs are poisoned with 0xee before the call.
        `nexpect` overrides the count passed to the ABI (for its argument checks)."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        if mode not in ("scan", "extract", "select"):
            raise ValueError("mode: scan, extract or select")
        sel, _nkeep = _jg_select(names) if names is not None else (None, None)
        out = _poisoned(ctypes.c_char, n)
        vals = _poisoned(JgClaims, n) if mode != "scan" else None
        sels = _poisoned(JgSelected, n) if mode == "select" else None
        self._claims_call("jg_claims_each", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          ctypes.byref(sel) if sel is not None else None, out,
                          ctypes.cast(vals, ctypes.c_void_p) if vals is not None else None,
                          ctypes.cast(sels, ctypes.c_void_p) if sels is not None else None)
        if mode == "scan":
            return out.raw[:n]
        if mode == "extract":
            return out.raw[:n], _records(JgClaims, vals, n)
        return out.raw[:n], _records(JgClaims, vals, n), _records(JgSelected, sels, n)

    def claims_paths(self, arena_bytes, jobs, expects, paths, nexpect=None, null=()):
        """jg_claims_paths: claims_each's selecting form for members named by path.
        `jobs`: (off, len, profile) triples; `expects`: a list of dicts as
        claims_scan takes one; `paths`: a list of paths, each a sequence of
        components (bytes) -> (codes, vals, sels) as claims_select returns them.
        The outputs are poisoned with 0xee before the call.  `nexpect` overrides
        the count passed to the ABI and `null` names arguments ("paths", "vals",
        "sels") to pass as NULL (both for its argument checks)."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        ps, _nkeep = _jg_paths(paths)
        out, vals, sels = _poisoned(ctypes.c_char, n), _poisoned(JgClaims, n), _poisoned(JgSelected, n)
        self._claims_call("jg_claims_paths", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          None if "paths" in null else ctypes.byref(ps), out,
                          None if "vals" in null else ctypes.cast(vals, ctypes.c_void_p),
                          None if "sels" in null else ctypes.cast(sels, ctypes.c_void_p))
        return out.raw[:n], _records(JgClaims, vals, n), _records(JgSelected, sels, n)

    def claims_match(self, arena_bytes, jobs, expects, paths, preds, nexpect=None, null=()):
        """jg_claims_match: claims_each's codes and, per job, the mask of the
        predicates that hold on the members `paths` reach.  `jobs`, `expects` and
        `paths` as claims_paths takes them; `preds`: a list of (path index, op,
        value bytes) with op one of PRED_* -> (codes: bytes, masks: list of int).
        Both outputs are poisoned with 0xee before the call.  `nexpect` overrides
        the count passed to the ABI and `null` names arguments ("paths", "preds",
        "codes", "masks") to pass as NULL (both for its argument checks)."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        ps, _nkeep = _jg_paths(paths)
        qs, _vkeep = _jg_preds(preds)
        out, masks = _poisoned(ctypes.c_char, n), _poisoned(ctypes.c_uint32, n)
        self._claims_call("jg_claims_match", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          None if "paths" in null else ctypes.byref(ps),
                          None if "preds" in null else ctypes.byref(qs),
                          None if "codes" in null else out,
                          None if "masks" in null else ctypes.cast(masks, ctypes.c_void_p))
        return out.raw[:n], list(masks[:n])

    def claims_match_args(self, arena_bytes, jobs, expects, paths, preds, args, nexpect=None, null=()):
        """jg_claims_match_args: claims_match with the jobs' own operands.  `preds`
        may hold the ops PRED_EQUALS_ARG, PRED_NUM_GE_ARG and PRED_NUM_LE_ARG (the
        value is one byte, the column) and PRED_NUM_GE / PRED_NUM_LE (the value is
        the bound as 8 little-endian bytes); `args`: pack_args' dict -> (codes:
        bytes, masks: list of int), both poisoned with 0xee before the call.  `null`
        names arguments ("paths", "preds", "args", "codes", "masks") or members of
        the operands ("bytes", "str", "num") to pass as NULL."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        ps, _nkeep = _jg_paths(paths)
        qs, _vkeep = _jg_preds(preds)
        ga, _akeep = _jg_args(args, null)
        out, masks = _poisoned(ctypes.c_char, n), _poisoned(ctypes.c_uint32, n)
        self._claims_call("jg_claims_match_args", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          None if "paths" in null else ctypes.byref(ps),
                          None if "preds" in null else ctypes.byref(qs),
                          None if "args" in null else ctypes.byref(ga),
                          None if "codes" in null else out,
                          None if "masks" in null else ctypes.cast(masks, ctypes.c_void_p))
        return out.raw[:n], list(masks[:n])

    def claims_match_hash(self, arena_bytes, jobs, expects, paths, preds, args=None, hargs=None, nexpect=None, null=()):
        """jg_claims_match_hash: claims_match_args with hash columns.  `preds` may
        also hold PRED_EQUALS_HASH (the value is one byte, the hash column) and
        PRED_IS_STRING (no value); `args`: pack_args' dict, or None for NULL (no
        plain columns); `hargs`: pack_hargs' dict, or None for NULL (no hash
        column) -> (codes: bytes, masks: list of int), both poisoned with 0xee
        before the call.  `null` names arguments ("paths", "preds", "codes",
        "masks") or members of the operands ("bytes", "str", "num", "hbytes",
        "hsrc") to pass as NULL."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        ps, _nkeep = _jg_paths(paths)
        qs, _vkeep = _jg_preds(preds)
        ga, _akeep = _jg_args(args, null) if args is not None else (None, None)
        gh, _hkeep = _jg_hargs(hargs, null) if hargs is not None else (None, None)
        out, masks = _poisoned(ctypes.c_char, n), _poisoned(ctypes.c_uint32, n)
        self._claims_call("jg_claims_match_hash", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          None if "paths" in null else ctypes.byref(ps),
                          None if "preds" in null else ctypes.byref(qs),
                          None if ga is None else ctypes.byref(ga),
                          None if gh is None else ctypes.byref(gh),
                          None if "codes" in null else out,
                          None if "masks" in null else ctypes.cast(masks, ctypes.c_void_p))
        return out.raw[:n], list(masks[:n])

    def set_load(self, set_id, members, seed=0, spans=None):
        """jg_set_load: set `set_id` of the context = `members` (a list of bytes),
        built under `seed`.  `spans` overrides the (off, len) rows handed to the ABI
        over the members' bytes back to back (for its argument checks)."""
        members = [bytes(m) for m in members]
        blob = b"".join(members)
        if spans is None:
            spans, o = [], 0
            for m in members:
                spans.append((o, len(m)))
                o += len(m)
        sp = (JgSArg * max(1, len(spans)))()
        for t, (off, ln) in zip(sp, spans):
            t.off, t.len = off, ln
        rc = lib().jg_set_load(self.h, int(set_id), blob or b"\0", len(blob), ctypes.cast(sp, ctypes.c_void_p),
                               len(spans), int(seed) & 0xffffffff)
        if rc != 0:
            raise JgError(f"jg_set_load rc={rc}: {self.error()}")

    def set_add(self, set_id, members, spans=None, want_added=True):
        """jg_set_add: adds `members` (a list of bytes) to the loaded set `set_id`
        on the device -> how many were not in it (None with want_added=False, which
        passes NULL).  `spans` as set_load takes it."""
        members = [bytes(m) for m in members]
        blob = b"".join(members)
        if spans is None:
            spans, o = [], 0
            for m in members:
                spans.append((o, len(m)))
                o += len(m)
        sp = (JgSArg * max(1, len(spans)))()
        for t, (off, ln) in zip(sp, spans):
            t.off, t.len = off, ln
        added = ctypes.c_uint32(0xeeeeeeee)
        rc = lib().jg_set_add(self.h, int(set_id), blob or b"\0", len(blob), ctypes.cast(sp, ctypes.c_void_p),
                              len(spans), ctypes.byref(added) if want_added else None)
        if rc != 0:
            raise JgError(f"jg_set_add rc={rc}: {self.error()}")
        return added.value if want_added else None

    def set_free(self, set_id):
        """jg_set_free"""
        rc = lib().jg_set_free(self.h, int(set_id))
        if rc != 0:
            raise JgError(f"jg_set_free rc={rc}: {self.error()}")

    def set_info(self, set_id):
        """jg_set_info -> {"n", "nslots", "maxprobe", "seed", "pool_bytes", "generation"}"""
        out = JgSetInfo()
        rc = lib().jg_set_info(self.h, int(set_id), ctypes.byref(out))
        if rc != 0:
            raise JgError(f"jg_set_info rc={rc}: {self.error()}")
        return {k: int(getattr(out, k)) for k, _ in JgSetInfo._fields_}

    def set_read(self, set_id):
        """jg_debug_set_read -> (slots: list of (hash, ref), pool: list of dwords) as they lie on the device"""
        info = self.set_info(set_id)
        ns, nd = info["nslots"], info["pool_bytes"] // 4
        slots, pool = (ctypes.c_uint32 * (2 * ns))(), (ctypes.c_uint32 * max(1, nd))()
        rc = lib().jg_debug_set_read(self.h, int(set_id), ctypes.cast(slots, ctypes.c_void_p), ns,
                                     ctypes.cast(pool, ctypes.c_void_p), nd)
        if rc != 0:
            raise JgError(f"jg_debug_set_read rc={rc}: {self.error()}")
        return [(slots[2 * k], slots[2 * k + 1]) for k in range(ns)], list(pool[:nd])

    def claims_match_set(self, arena_bytes, jobs, expects, paths, preds, args=None, hargs=None, sets=None, nexpect=None,
                         null=(), nsets=None):
        """jg_claims_match_set: claims_match_hash with set predicates.  `preds` may
        also hold PRED_IN_SET and PRED_ELEMENT_IN_SET (the value is one byte, an
        index into `sets`); `sets`: the ids of loaded sets the call names, or None
        for NULL -> (codes: bytes, masks: list of int), both poisoned with 0xee
        before the call.  `nsets` overrides the count passed to the ABI; `null` as
        claims_match_hash takes it."""
        n = len(jobs)
        es, _keep = _jg_expects(expects)
        ps, _nkeep = _jg_paths(paths)
        qs, _vkeep = _jg_preds(preds)
        ga, _akeep = _jg_args(args, null) if args is not None else (None, None)
        gh, _hkeep = _jg_hargs(hargs, null) if hargs is not None else (None, None)
        gs = _jg_setargs(sets, nsets) if sets is not None else None
        out, masks = _poisoned(ctypes.c_char, n), _poisoned(ctypes.c_uint32, n)
        self._claims_call("jg_claims_match_set", arena_bytes, _cjobs(jobs), n, es,
                          len(expects) if nexpect is None else nexpect,
                          None if "paths" in null else ctypes.byref(ps),
                          None if "preds" in null else ctypes.byref(qs),
                          None if ga is None else ctypes.byref(ga),
                          None if gh is None else ctypes.byref(gh),
                          None if gs is None else ctypes.byref(gs),
                          None if "codes" in null else out,
                          None if "masks" in null else ctypes.cast(masks, ctypes.c_void_p))
        return out.raw[:n], list(masks[:n])

    def set_chunk(self, jobs):
        if lib().jg_set_chunk(self.h, jobs) != 0:
            raise JgError("jg_set_chunk: chunk must be >= 64 jobs")

    def set_zero_copy(self, enable, max_jobs=0):
        """jg_set_zero_copy: class-major zero-copy plans for mixed batches whose
        arena is a PinnedBuffer (off by default), and the jobs per plan."""
        if lib().jg_set_zero_copy(self.h, 1 if enable else 0, max_jobs) != 0:
            raise JgError("jg_set_zero_copy: max_jobs must be 0 or >= 64")

    def set_table_budget(self, nbytes):
        """jg_set_table_budget: HBM for all key comb tables (applies at the next load_keys)."""
        if lib().jg_set_table_budget(self.h, int(nbytes)) != 0:
            raise JgError("jg_set_table_budget failed")

    def submit(self, arena: Arena):
        """jg_submit; returns a Pending whose wait() gives the verdict bytes."""
        return Pending(self, arena)

    # ---- device-resident batches (bench)
    def stage(self, arena: Arena, slot=0):
        h = ctypes.c_void_p()
        buf = bytes(arena.buf) or b"\0"
        rc = lib().jg_batch_stage(self.h, slot, buf, len(arena.buf), arena.tok_array(), len(arena.toks),
                                  ctypes.byref(h))
        if rc != 0:
            raise JgError(f"jg_batch_stage rc={rc}: {self.error()}")
        return Batch(self, h, len(arena.toks))


class Pending:
    """One jg_submit in flight (buffers kept alive until wait())."""

    def __init__(self, ctx, arena):
        self.ctx = ctx
        self.n = len(arena.toks)
        self.buf = ctypes.create_string_buffer(bytes(arena.buf) or b"\0", max(1, len(arena.buf)))
        self.toks = arena.tok_array()
        self.out = (ctypes.c_uint8 * max(1, self.n))()
        self.t = ctypes.c_void_p()
        rc = lib().jg_submit(ctx.h, self.buf, len(arena.buf), self.toks, self.n, self.out, ctypes.byref(self.t))
        if rc != 0:
            raise JgError(f"jg_submit rc={rc}: {ctx.error()}")

    def wait(self):
        rc = lib().jg_wait(self.ctx.h, self.t)
        self.t = None
        if rc != 0:
            raise JgError(f"jg_wait rc={rc}: {self.ctx.error()}")
        return bytes(self.out[:self.n])


class PinnedBuffer:
    """Page-locked host memory from jg_host_alloc (hipHostMalloc)."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.ptr = lib().jg_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise JgError("jg_host_alloc failed")

    def bytes(self):
        return ctypes.string_at(self.ptr, self.n)

    def free(self):
        if self.ptr:
            lib().jg_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Batch:
    def __init__(self, ctx, h, n):
        self.ctx, self.h, self.n = ctx, h, n

    def run(self, want_verdicts=False):
        out = (ctypes.c_uint8 * max(1, self.n))() if want_verdicts else None
        rc = lib().jg_batch_run(self.ctx.h, self.h, out)
        if rc != 0:
            raise JgError(f"jg_batch_run rc={rc}: {self.ctx.error()}")
        return bytes(out[:self.n]) if want_verdicts else None

    def enqueue(self, pinned_verdicts=None):
        """Enqueue one run without waiting; verdicts land in `pinned_verdicts`
        (a PinnedBuffer) once sync() returns."""
        ptr = pinned_verdicts.ptr if pinned_verdicts is not None else None
        rc = lib().jg_batch_enqueue(self.ctx.h, self.h, ptr)
        if rc != 0:
            raise JgError(f"jg_batch_enqueue rc={rc}: {self.ctx.error()}")

    def sync(self):
        rc = lib().jg_batch_sync(self.ctx.h, self.h)
        if rc != 0:
            raise JgError(f"jg_batch_sync rc={rc}: {self.ctx.error()}")

    def exceptions(self):
        """Per-class count of tokens the last run sent down the exact ECDSA path."""
        c = (ctypes.c_uint32 * 8)()
        n = lib().jg_batch_exceptions(self.h, c, 8)
        if n < 0:
            raise JgError(f"jg_batch_exceptions rc={n}: {self.ctx.error()}")
        return list(c)

    def kernel_times(self):
        names = (ctypes.c_char_p * 64)()
        ms = (ctypes.c_float * 64)()
        n = lib().jg_batch_kernel_times(self.h, names, ms, 64)
        return [(names[i].decode(), ms[i]) for i in range(min(n, 64))]

    def free(self):
        if self.h:
            lib().jg_batch_free(self.ctx.h, self.h)
            self.h = None
