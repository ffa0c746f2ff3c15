"""The declared plan of tests/test_gpu_k2_forms.py: which databases, which batches, which settings, and which instantiation(s) of
the COBS kernel every case must launch.  No GPU and no library is needed to import it: test_k2_forms_plan_cpu.py checks on every
machine that the plan names every instantiation kmcp_amd/csrc/k2_cobs.hip can launch.

A form is the tuple (kind, lpr, lprb, npl, multi, group_rows) that `Database.last_k2_launches()` reports (without the workgroup
count): kind "plain" = k2_cobs<LPR, NPL, MULTI, false, GR>, "split" = k2_cobs<LPR, 16, MULTI, true> (the chunked long-query form),
"pair" = k2_cobs_pair<64, LPRB, 16, MULTI>.

The expectations are NOT read from the library: `expect()` below restates the dispatch rules of kmcp_amd/csrc/k2_plan.hpp (k2_row_parts:
row pitch -> lane classes; k2_ask_long / k2_plan: longest query -> planes, index size -> rows per group, chunked / pair decisions, the
kernel that runs) from the point of view of a test that knows its database and its batch.  A change of any of those rules moves a
case onto another form and turns its witness assertion red — that is the point; test_k2_forms_plan_cpu.py holds this restatement
against the header compiled for the host, case by case."""
import itertools
from collections import namedtuple

K = 21  # k-mer size of every database of the plan

LPRS = (4, 8, 16, 32, 64)
# ---- every instantiation the launchers of k2_cobs.hip can launch (the product of their parameter sets) ------------------------
ALL_FORMS = frozenset(
    [("plain", l, 0, p, m, 8) for l, p, m in itertools.product(LPRS, (8, 10, 16, 24), (False, True))] +      # plain, 8 rows: 40
    [("plain", l, 0, p, m, 4) for l, p, m in itertools.product(LPRS, (8, 10), (False, True))] +              # plain, 4 rows: 20
    [("split", l, 0, 16, m, 8) for l, m in itertools.product(LPRS, (False, True))] +                          # chunked: 10
    [("pair", 64, lb, 16, m, 8) for lb, m in itertools.product((4, 8, 16, 32), (False, True))])              # pair: 8
assert len(ALL_FORMS) == 78

# forms no database reaches by the default rules; the override that reaches them
OVERRIDE_ONLY = {
    ("pair", 64, 4, 16, True, 8): "KMCPG_ROW_ALIGN=64 at open (databases with several hash functions get a 128-byte row pitch: no 64-byte remainder)",
}
# ... and, for indexes below 4 GiB (everything here but the `big8` database), every 4-row form: KMCPG_GROUP_ROWS=4


# ---- databases -------------------------------------------------------------------------------------------------------------
# cols: columns per block (never a multiple of 8: padding bits in the last byte); step: sigs_step (0 = equal NumSigs, the blocks
# fuse into one group whose segments start at byte offsets that are not multiples of 16); stride1 / stridem: the row pitch the
# group gets with one / with several hash functions (64- / 128-byte alignment above 128 bytes).
Layout = namedtuple("Layout", "name cols blocks step stride1 stridem")
LAYOUTS = [
    Layout("n4s", 100, 4, 7, 16, 16),          # 13-byte rows: three of the four lanes past the row
    Layout("n4", 309, 2, 7, 64, 64),
    Layout("n8", 997, 2, 7, 128, 128),
    Layout("n16a", 1499, 2, 7, 192, 256),
    Layout("n16b", 2045, 2, 7, 256, 256),
    Layout("n32a", 2049, 2, 7, 320, 384),
    Layout("n32b", 4093, 2, 7, 512, 512),
    Layout("n64p", 4100, 2, 7, 576, 640),      # a part-filled 64-lane tile
    Layout("n64f", 8189, 2, 7, 1024, 1024),    # a full one
    Layout("p4", 8501, 2, 7, 1088, 1152),      # 64 + 4 (several hashes: 64 + 8)
    Layout("p8", 8997, 2, 7, 1152, 1152),      # 64 + 8
    Layout("p16", 9981, 2, 7, 1280, 1280),     # 64 + 16
    Layout("p32", 11997, 2, 7, 1536, 1536),    # 64 + 32
    Layout("t3", 13001, 3, 7, 1664, 1664),     # 64 + 32 + 8 with one hash function (640-byte remainder), two 64-lane tiles otherwise
    # several blocks of equal NumSigs side by side in one group
    Layout("f4", 100, 3, 0, 64, 64),           # 3 x 13 bytes
    Layout("f8", 309, 3, 0, 128, 128),         # 3 x 39
    Layout("f16", 499, 3, 0, 192, 256),        # 3 x 63
    Layout("f32", 997, 3, 0, 384, 384),        # 3 x 125
    Layout("f64", 2501, 3, 0, 960, 1024),      # 3 x 313
    Layout("fp16", 3301, 3, 0, 1280, 1280),    # 3 x 413: 64 + 16
]
LAYOUT = {l.name: l for l in LAYOUTS}

NUM_SIGS = 30011      # rows of block 0 ("tens of thousands": the point is forms, not size)
AND_DENSITY = 0.3     # share of set bits in the AND of a k-mer's h rows

Db = namedtuple("Db", "key layout nh open_env num_sigs")


def _db(layout, nh, open_env=(), num_sigs=NUM_SIGS):
    key = "%s-h%d" % (layout, nh) + "".join("-%s%s" % (k.replace("KMCPG_", "").lower(), v) for k, v in open_env)
    return Db(key, layout, nh, tuple(open_env), num_sigs)


DBS = [_db(l.name, nh) for l in LAYOUTS for nh in (1, 3)]
DBS += [_db("n8", 2), _db("p16", 2), _db("n4", 4), _db("p32", 4)]       # 2 and 4 hash functions: a narrow and a wide layout each
DBS += [_db("p4", 3, (("KMCPG_ROW_ALIGN", "64"),))]                      # override only: the 64 + 4 pair with several hash functions
# the 4-row forms by the default rule: 128-byte rows, 4.35 GB resident (>= 4 GiB); skipped when HBM is short
BIG = Db("big8-h1", "big8", 1, (), 34_000_000)
LAYOUT["big8"] = Layout("big8", 1021, 1, 0, 128, 128)
DB = {d.key: d for d in DBS + [BIG]}


def stride_of(db):
    l = LAYOUT[db.layout]
    if dict(db.open_env).get("KMCPG_ROW_ALIGN") == "64":
        return l.stride1
    return l.stride1 if db.nh == 1 else l.stridem


def lane_classes(stride, nh, open_env=()):
    """k2_row_parts: whole 1-KiB tiles -> 64 lanes; the remainder -> the narrowest lane form that covers it (a 640-byte remainder of a
    single-hash database: 32 + 8).  Lane classes in the order the database gets them, and the slots (tiles) of one group per class."""
    env = dict(open_env)
    full, rem = divmod(stride, 1024)
    parts = [64] * full
    st = int(env.get("KMCPG_SPLIT_TILES", -1))
    split = 256 < rem <= 896 and bin(rem // 64).count("1") <= 3 and (st == 2 or (st == 1 and nh > 1) or (st < 0 and rem == 640 and nh == 1))
    if rem and split:
        left = rem
        for part in (512, 256, 128, 64):
            if left >= part:
                parts.append(part // 16)
                left -= part
    elif rem:
        lpr32 = env.get("KMCPG_LPR32") != "0"
        parts.append(4 if rem <= 64 else 8 if rem <= 128 else 16 if rem <= 256 else 32 if (rem <= 512 and lpr32) else 64)
    classes = []
    for p in parts:
        if p not in classes:
            classes.append(p)
    return classes, {c: parts.count(c) for c in classes}


# ---- batches: one per plane class ----------------------------------------------------------------------------------------------
# NumKmers of the queries (read length = n + K - 1; n = 0: a read one base shorter than K).  Ragged on purpose: the units that
# share a wave have different n.  Every batch holds the class's exact maximum (254 / 1 022 / 65 534) and the batch above it the next
# class's minimum (255 / 1 023 / 65 535).  Sizes are not multiples of 4 * G units for any G.  The 8- and 10-plane batches end in a
# cluster of queries near the class's maximum: a min_matched that lets an eighth of all (query, column) pairs pass then sits in the
# body of the cluster's count distribution (n = 1 022 at density 0.3: mean 307, s.d. 15, P(count = cmin) ~ 0.027 per column), which is
# what puts more than one column per query exactly at cmin and at cmin - 1 even on the 300-column databases.
_RAGGED = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
BATCH_N = {
    8: _RAGGED + [100, 127, 128, 129, 130, 130, 130, 131, 150, 150, 191, 192, 193, 200, 221, 240, 248, 250, 252, 253, 254, 254],
    10: _RAGGED + [127, 128, 129, 130, 255, 255, 256, 257, 300, 383, 384, 385, 500, 511, 512, 513, 700, 767, 900, 1000, 1005, 1010, 1015, 1018, 1020, 1021, 1022, 1022],
    # one query at the top of the range (its reference is a 65 534-row gather per block and hash function), a handful between
    16: _RAGGED + [130, 255, 1023, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 65534],
    # 24 planes: one query at the class's minimum; the rest of the batch rides along on 24 planes
    24: _RAGGED + [130, 255, 1023, 2049, 4097, 65535],
}
SPLIT_DEFAULT = 2048   # KMCPG_SPLIT_MIN when unset
SPLIT_SMALL = 16       # sends most of every batch to the chunked form: with KMCPG_SPLIT_CHUNK=64 a query spans 1, 2 or many chunks


def planes_for(max_n):
    return 8 if max_n <= 254 else 10 if max_n <= 1022 else 16 if max_n <= 65534 else 24


def expect(db, batch, env, index_bytes=0):
    """The launches (sorted list of forms) kmcpg_query_device must make for batch `batch` of database `db` under `env`.
    `batch`: a plane class of BATCH_N, or the NumKmers of a batch of the caller's own (tests/k2_overflow.py)."""
    ns = BATCH_N[batch] if isinstance(batch, int) else list(batch)
    classes, slots = lane_classes(stride_of(db), db.nh, db.open_env)
    multi = db.nh > 1
    groups = 1 if LAYOUT[db.layout].step == 0 else LAYOUT[db.layout].blocks
    total_slots = groups * sum(slots.values())
    max_n = max(ns)
    sm_env = "KMCPG_SPLIT_MIN" in env
    split_min = int(env.get("KMCPG_SPLIT_MIN", SPLIT_DEFAULT))
    ask = split_min > 0 and max_n > split_min and (sm_env or max_n > 32768 or len(ns) * total_slots <= 16384)
    longs = [n for n in ns if n > split_min] if ask else []
    if longs and not sm_env and len(longs) * total_slots >= 1536 and max(longs) <= 65534:
        longs = []
    max_short = max_n if not ask else (split_min if longs else max(max(longs, default=0), split_min))
    npl = planes_for(max_short)
    prune = int(env.get("KMCPG_PRUNE", 1))
    gr = 4 if (prune and npl <= 10 and index_bytes >= (4 << 30)) else 8
    if "KMCPG_GROUP_ROWS" in env:
        gr = 4 if int(env["KMCPG_GROUP_ROWS"]) == 4 else 8
    out = []
    pair = npl >= 16 and len(classes) == 2 and classes[0] == 64 and classes[1] < 64 and env.get("KMCPG_PAIR") != "0"
    if pair and npl == 16 and gr != 4:        # no pair kernel at 24 planes or under the 4-row setting
        out.append(("pair", 64, classes[1], 16, multi, 8))
    else:
        for c in classes:
            out.append(("plain", c, 0, npl, multi, 4 if (npl <= 10 and gr == 4) else 8))   # no 4-row kernels at 16 / 24 planes
    if longs:
        out += [("split", c, 0, 16, multi, 8) for c in classes]
    return sorted(out)


# ---- the matrix ------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id db batch knob env expect")


def _knobs(db, batch):
    classes, _ = lane_classes(stride_of(db), db.nh, db.open_env)
    two = len(classes) == 2 and classes[0] == 64
    s0 = {"KMCPG_SPLIT_MIN": "0"}
    ks = [("default", {})]
    if batch in (8, 10):
        ks += [("gr4", {"KMCPG_GROUP_ROWS": "4"}), ("gr8", {"KMCPG_GROUP_ROWS": "8"}), ("prune0", {"KMCPG_PRUNE": "0"}), ("split0", s0)]
    elif batch == 16:
        ks += [("split0", s0), ("split0-prune0", dict(s0, KMCPG_PRUNE="0")), ("split0-gr4", dict(s0, KMCPG_GROUP_ROWS="4"))]
    else:
        ks += [("split0", s0), ("split0-prune0", dict(s0, KMCPG_PRUNE="0"))]
    ks += [("split%d-chunk64" % SPLIT_SMALL, {"KMCPG_SPLIT_MIN": str(SPLIT_SMALL), "KMCPG_SPLIT_CHUNK": "64"}),
           ("split%d" % SPLIT_SMALL, {"KMCPG_SPLIT_MIN": str(SPLIT_SMALL)})]
    if batch >= 16 and two:
        ks += [("split0-pair0", dict(s0, KMCPG_PAIR="0"))]
    if batch >= 16 and 64 in classes:
        ks += [("split0-tail0", dict(s0, KMCPG_TAIL_SECTORS="0"))]
    return ks


def _cases():
    out = []
    for db in DBS:
        for batch in (8, 10, 16, 24):
            for knob, env in _knobs(db, batch):
                out.append(Case("%s-%dp-%s" % (db.key, batch, knob), db.key, batch, knob, env, tuple(expect(db, batch, env))))
    # cheap extras on references that exist anyway: same list under the layout / load / cadence knobs (one lane layout per knob)
    extras = [("n4", {"KMCPG_SLOT_MAJOR": "0"}), ("n8", {"KMCPG_SLOT_MAJOR": "2"}), ("f16", {"KMCPG_SLOT_MAJOR": "2"}), ("n32a", {"KMCPG_SLOT_MAJOR": "0"}),
              ("n64p", {"KMCPG_NT_LOADS": "0"}), ("f8", {"KMCPG_NT_LOADS": "0"}),
              ("n16a", {"KMCPG_PRUNE_EVERY": "2"}), ("f32", {"KMCPG_PRUNE_EVERY": "4"}), ("p8", {"KMCPG_PRUNE_EVERY": "8"}), ("n4s", {"KMCPG_PRUNE_EVERY": "2"})]
    for lay, env in extras:
        for nh in (1, 3):
            db = DB["%s-h%d" % (lay, nh)]
            knob = "-".join("%s%s" % (k.replace("KMCPG_", "").lower(), v) for k, v in env.items())
            out.append(Case("%s-8p-%s" % (db.key, knob), db.key, 8, knob, env, tuple(expect(db, 8, env))))
    # the 4-row forms by the default rule (index >= 4 GiB), no override
    for batch in (8, 10):
        out.append(Case("%s-%dp-default" % (BIG.key, batch), BIG.key, batch, "default", {}, tuple(expect(BIG, batch, {}, index_bytes=BIG.num_sigs * 128))))
    return out


CASES = _cases()


def fmt(form):
    kind, lpr, lprb, npl, multi, gr = form
    m = "true" if multi else "false"
    if kind == "pair":
        return "k2_cobs_pair<64,%d,%d,%s>" % (lprb, npl, m)
    return "k2_cobs<%d,%d,%s,%s,%d>" % (lpr, npl, m, "true" if kind == "split" else "false", gr)
