"""The case table of the MFMA GEMM kernels (csrc/mmq_rgemm.hip, mmq_gemm.hip, mmq_skinny.hip,
mmq_kstream.hip), built from the library itself.

built_kernels() reads which kernels the library holds: the link keeps one local `__device_stub__<kernel>`
symbol per instantiation, with its integer template arguments in the mangled name, and the ELF symbol
table is parsed here (kernel NAMES only; no device code is read).  The plan query (gq_debug_gemm_plan,
kernels._lib.gemm_plan) says which kernels a call launches and in which run-time form.  table() asks the
plan query -- host only, GQ_CUS set -- over the types, both activation forms, the token counts of every
token tile, K in whole super-blocks and the tuning vectors that reach each family, first planned for the
whole chip (CUS = 256), then for SMALL_CUS and (single matrices) TINY_CUS compute units, and keeps per (kernel, run-time form,
token count) the call of smallest K -- the q8_1 call before the fp8 one, which is therefore kept where the kernel
or its form is the fp8 variant's own (AQ = 2, the skinny kernel at 1..4 tokens): tests/test_gemm_cases_host.py proves from it that
every kernel of the inventory is reached or listed in UNREACHED, tests/test_gpu_gemm_cases.py runs every
case.

A new GEMM kernel, token tile, case set or block type belongs here (VECTORS, SET_ITEM) before it is done."""
import collections
import functools
import os
import re
import struct

import kernels._lib as kl

M = 293          # rows: two 256-row tiles (three of 128), the last of 37 rows -- odd, and a ragged 16-row group
M16 = 304        # the K-chunked stream needs M % 16 == 0
E, S = 3, 2      # the sorted entry: three experts, two slots per token
CUS = 256        # the chip the table is planned for
SMALL_CUS = 8    # ... for a small one: grids of several rounds, persistent workgroups with several units, stream-K
                 # workgroups that span tiles (a grouped launch is refused beyond tiles == cus: 6 of its 8 here)
TINY_CUS = 4     # ... and, the single-matrix entries alone, for one with no more CUs than the call has tiles: the
                 # planners' `tiles >= cus` branch (one split by the auto rule).  At these rows and tokens the
                 # largest tile grid is 3 x 2 (128-row tiles) or 2 x 2 (256-row tiles), so 8 never takes it.
RAGGED = (5, 17, 33, 129)   # the token counts of the grouped case sets 1..3 (set 0 runs every count)
FMTS = ("q8_0", "q4_k", "q6_k", "q5_k", "q3_k", "q2_k", "q4_0")
FMT_OF = {v: k for k, v in kl.TYPES.items()}
# a ragged and a full token tile per tile size (129: a second 128-token tile holding one token)
TOKENS = (5, 16, 17, 32, 33, 64, 65, 128, 129)
FP8_SKINNY_TOKENS = (1, 2, 3, 4)   # the fp8 variant has no GEMV: its 1..4 tokens take the skinny kernel
KS = tuple(range(256, 4352 + 1, 256)) + (8192, 16640, 20480)
KS_SHORT = (256, 512, 768, 1024, 2048)
FAMILIES = ("rgemm_kernel", "sgemm_kernel", "sgemm_id_kernel", "sgemm_grouped_kernel", "gemm_kernel", "skinny_kernel",
            "kstream_kernel")
# the split-K sums: launched beside a family's kernel, reached by that family's cases
REDUCES = ("gemm_reduce_f16_kernel", "gemm_reduce_kernel", "reduce_grouped_kernel", "kstream_reduce_kernel")
# a grouped launch's second item: the smallest matrix of the type that defines sgemm_grouped_kernel's case
# set (FmtInfo::sgemm_set; set 0 has no such type: Q4_K)
SET_ITEM = {0: ("q4_k", 5, 256), 1: ("q3_k", 5, 256), 2: ("q2_k", 5, 256), 3: ("q4_0", 5, 256)}
KSTREAM_ITEM = ("q4_k", 16, 256)   # ... and of the K-chunked stream's grouped launch

# name: the kernel template; args: its integer template arguments as the symbol table has them --
#   rgemm_kernel (F, NB, AQ, ES)   sgemm_kernel, sgemm_id_kernel (F, NB)   sgemm_grouped_kernel (NB, SET)
#   reduce_grouped_kernel (NB,)    gemm_kernel (F, NB, RG, 0, AM, NL, AQ)  gemm_reduce[_f16]_kernel (NB, RG)
#   skinny_kernel (F, NT, RG, 2)   kstream_kernel (NB, CWM)                kstream_reduce_kernel ()
Kernel = collections.namedtuple("Kernel", "name args")
# one call: entry point, activation form, the tuning vector's name, GQ_CUS, the (type name, M, K) items, N
Call = collections.namedtuple("Call", "entry act vector cus items N")
# a call and what it is kept for: covers = the (Kernel, form) pairs it is the smallest call of
Case = collections.namedtuple("Case", "call family covers")

_OFF = dict(GQ_RGEMM=0, GQ_SGEMM=0, GQ_SKINNY=0, GQ_KSTREAM=0)


def _vectors():
    """(name, tuning, entries, K list, row count): the tuning vectors that reach each family."""
    v = [("default", {}, ("ex", "prepared", "id_sorted", "grouped_prepared"), KS, M),
         ("default-m16", {}, ("ex", "prepared", "grouped_prepared", "grouped_ex"), KS, M16)]
    for es in (0, 1):
        for ilc in (0, 1):
            v.append((f"rgemm-es{es}-ilc{ilc}", dict(GQ_RGEMM=1, GQ_KSTREAM=0, GQ_RGEMM_ESTORE=es, GQ_RGEMM_ILC=ilc),
                      ("ex", "prepared"), KS_SHORT, M))
    sg = dict(_OFF, GQ_SGEMM=1)
    for sp in (0, 1, 3, 4):
        for full in (0, 1):
            for ilc in (0, 1):
                v.append((f"sgemm-s{sp}-full{full}-ilc{ilc}", dict(sg, GQ_SGEMM_SPLITS=sp, GQ_SGEMM_FULL=full, GQ_RGEMM_ILC=ilc),
                          ("prepared", "id_sorted", "grouped_prepared"), KS, M))
    for full in (0, 1):
        for ilc in (0, 1):
            v.append((f"sgemm-streamk-full{full}-ilc{ilc}",
                      dict(sg, GQ_SGEMM_STREAMK=1, GQ_SGEMM_FULL=full, GQ_RGEMM_ILC=ilc), ("prepared", "grouped_prepared"), KS, M))
    for rg in (1, 2, 3, 4):
        v.append((f"skinny-rg{rg}", dict(_OFF, GQ_SKINNY=1, GQ_SKINNY_RG=rg), ("ex", "prepared"), KS_SHORT, M))
    v.append(("kstream", dict(GQ_KSTREAM=1), ("ex", "prepared", "grouped_prepared", "grouped_ex"), KS, M16))
    for rg in (1, 2):
        for sp in (0, 1, 2):
            for part in (0, 1):
                for i8 in (0, 1):
                    for aq in (0, 1):
                        v.append((f"gemm-rg{rg}-s{sp}-{'f32' if part else 'f16'}-i8{i8}-aq{aq}",
                                  dict(_OFF, GQ_GEMM_RG=rg, GQ_GEMM_SPLITS=sp, GQ_GEMM_PARTIAL=part, GQ_GEMM_I8=i8, GQ_GEMM_AQ=aq),
                                  ("ex", "prepared"), KS_SHORT, M))
    return v


VECTORS = _vectors()
TUNING = {name: tuning for name, tuning, _, _, _ in VECTORS}

# Kernels the inventory has and that no call reaches under any vector above, at either GQ_CUS (the
# reasons: DESIGN.md, "The GEMM case table"; tests/test_gemm_cases_host.py asserts that no sweep selects
# them).  All are gemm_kernel<F, NB, RG, 0, AM, NL, AQ> of mmq_gemm.hip:
#   <F, NB, 1, 0, AF_F16, 0, 0> (12): plan_gemm sets loaders = 4 exactly when act == AF_F16 && rg == 1, so
#       the 128-row fp16 form always runs with its four loader waves (NL = 4);
#   <F, 8, 2, 0, AF_F16, 4, 0> (2: Q4_K, Q6_K): for the same reason the 256-row form never has loader waves;
#   <F, 4, 1, 0, AF_F16, 4, 1> (3): gemm_aq_ok admits in-kernel quantization up to nb = 2.
# They stay built; removing them would be a pure deletion in mmq_gemm.hip launch_fmt.
UNREACHED = ([Kernel("gemm_kernel", (f, nb, 1, 0, 0, 0, 0)) for f in (0, 1, 2) for nb in (1, 2, 4, 8)] +
             [Kernel("gemm_kernel", (f, 8, 2, 0, 0, 4, 0)) for f in (1, 2)] +
             [Kernel("gemm_kernel", (f, 4, 1, 0, 0, 4, 1)) for f in (0, 1, 2)])


# ---- the inventory: the library's symbol table ----
def _symbols(path):
    """Every name of the ELF64 little-endian file's .symtab sections."""
    with open(path, "rb") as f:
        d = f.read()
    assert d[:4] == b"\x7fELF" and d[4] == 2 and d[5] == 1, "an ELF64 little-endian file"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ != 2:  # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for i in range(size // entsize):
            st_name, = struct.unpack_from("<I", d, off + i * entsize)
            out.append(d[stroff + st_name:d.index(b"\0", stroff + st_name)].decode())
    return out


_STUB = re.compile(r"(\d+)__device_stub__")


def stub_kernel(symbol):
    """Kernel of a mangled `__device_stub__` symbol, e.g. ..N_126__device_stub__gemm_kernelILi0ELi1ELi1ELi0ELi0ELi4ELi1EE...
    -> ("gemm_kernel", (0, 1, 1, 0, 0, 4, 1)); None for any other symbol."""
    m = _STUB.search(symbol)
    if not m:
        return None
    digits, at = m.group(1), m.end(1)
    for k in range(len(digits) - 1, -1, -1):  # ("N_127__device_stub__...": the name's length is 26, not 126)
        n = int(digits[k:])
        if n > 15 and re.fullmatch(r"\w+", symbol[at:at + n]) and symbol[at + n:at + n + 1] in ("I", "E"):
            break
    else:
        return None
    rest = symbol[at + n:]
    args = ()
    if rest.startswith("I"):
        t = re.match(r"I((?:L[ib]n?\d+E)+)E", rest)
        if not t:
            return None
        args = tuple(int(a.replace("n", "-")) for a in re.findall(r"L[ib](n?\d+)E", t.group(1)))
    return Kernel(symbol[at + 15:at + n], args)


@functools.lru_cache(maxsize=None)
def built_kernels():
    """{family or reduce name: sorted [Kernel]} of the four GEMM files, from lib/libgguf_mmq.so's symbol table
    (the objects under build/obj when the library was stripped)."""
    paths = [kl.LIB_PATH]
    obj = os.path.join(os.path.dirname(kl.LIB_DIR), "build", "obj")
    paths += [os.path.join(obj, f"mmq_{n}.o") for n in ("rgemm", "gemm", "skinny", "kstream")]
    for group in (paths[:1], paths[1:]):
        if not all(os.path.exists(p) for p in group):
            continue
        found = {stub_kernel(s) for p in group for s in _symbols(p)} - {None}
        out = {n: sorted(k for k in found if k.name == n) for n in FAMILIES + REDUCES}
        if any(out.values()):
            return out
    raise RuntimeError("no __device_stub__ symbols in the library or its objects")


# ---- a plan entry's kernel and run-time form ----
def kernel_of(p):
    """The instantiation a plan entry (kl.GemmPlan) names."""
    name = kl.GEMM_KERNELS[p.kernel]
    args = {"rgemm_kernel": (p.fmt, p.nb, p.aq, p.es), "sgemm_kernel": (p.fmt, p.nb), "sgemm_id_kernel": (p.fmt, p.nb),
            "sgemm_grouped_kernel": (p.nb, p.set), "reduce_grouped_kernel": (p.nb,),
            "gemm_kernel": (p.fmt, p.nb, p.rg, 0, p.am, p.nl, p.aq), "gemm_reduce_f16_kernel": (p.nb, p.rg),
            "gemm_reduce_kernel": (p.nb, p.rg), "skinny_kernel": (p.fmt, p.nb, p.rg, 2), "kstream_kernel": (p.nb, p.cwm),
            "kstream_reduce_kernel": ()}[name]
    return Kernel(name, args)


def form_of(p, cus):
    """The run-time form of a plan entry: the branches of the kernel it takes that the template arguments
    do not say.  `rounds`: more workgroups (skinny, kstream: units) than one round of the planned chip;
    `chipfull`: at least as many tiles as the planned chip has CUs (plan_gemm's and plan_sgemm's one-split rule).
    The grouped kernel's in-launch sum is a form in case set 0 only (the sets share that code)."""
    name = kl.GEMM_KERNELS[p.kernel]
    split = "split" if p.splits > 1 else "whole"
    rounds = ("rounds",) if (p.tiles_m > p.blocks if name in ("skinny_kernel", "kstream_kernel") else p.blocks > cus) else ()
    if name in ("rgemm_kernel", "sgemm_kernel", "gemm_kernel") and p.tiles_m * p.tiles_n >= cus:
        rounds += ("chipfull",)
    if name == "rgemm_kernel":
        return (split,) + (("ilc",) if p.ilc else ()) + rounds
    if name == "sgemm_kernel":
        # (the split-major order: one form whatever the chip -- its shapes cost a CPU ideal of up to a second each)
        return (split, f"order{p.order}") + (("full",) if p.full else ()) + (rounds if p.order != 2 else ())
    if name == "sgemm_id_kernel":
        return (("full",) if p.full else ())
    if name == "sgemm_grouped_kernel":
        return (FMT_OF[p.fmt], split) + (("streamk",) if p.streamk else ()) + \
               (("ilc",) if p.ilc and p.splits > 1 and p.set == 0 else ()) + (("full",) if p.full else ())
    if name == "gemm_kernel":
        return (split,) + ((("pf16",) if p.pf16 else ("pf32",)) if p.splits > 1 else ()) + rounds
    if name == "kstream_kernel":
        return (f"aq{p.aq}", split) + rounds
    if name == "skinny_kernel":
        return rounds
    return ()


def items_of(entry, fmt, rows, K, set_=0):
    """The (type name, M, K) list of a call: the matrix under test, in a grouped launch beside the set's item."""
    head = [(fmt, rows, K)]
    if entry == "grouped_prepared":
        return tuple(head + [SET_ITEM[set_]])
    if entry == "grouped_ex":
        return tuple(head + [KSTREAM_ITEM])
    return tuple(head)


def plan(call):
    """The plan query's entries for the call under the CURRENT tuning (the caller sets call.vector and call.cus)."""
    kw = dict(E=E, S=S) if call.entry == "id_sorted" else {}
    return kl.gemm_plan(call.entry, [(kl.TYPES[f], m, k) for f, m, k in call.items], call.N, call.act, **kw)


def under_test(entries):
    """The entries that compute the matrix under test (item 0) or serve its launch (item -1)."""
    return [p for p in entries if p.item in (0, -1)]


def set_vector(name, cus):
    kl.reset_tuning()
    for k, v in TUNING[name].items():
        kl.set_tuning(k, v)
    kl.set_tuning("GQ_CUS", cus)


def fp8_ok(fmt):
    return fmt in ("q8_0", "q4_k", "q6_k")


def _calls(name, entries, ks, rows, cus):
    for entry in entries:
        sets = sorted(SET_ITEM) if entry == "grouped_prepared" else (0,)
        for fmt in FMTS:
            for act in ("q8_1", "fp8"):
                if act == "fp8" and not fp8_ok(fmt):
                    continue
                toks = TOKENS + (FP8_SKINNY_TOKENS if act == "fp8" and entry in ("ex", "prepared") else ())
                for st in sets:
                    for N in (toks if st == 0 else RAGGED):
                        for K in ks:
                            yield Call(entry, act, name, cus, items_of(entry, fmt, rows, K, st), N)


Table = collections.namedtuple("Table", "cases best selected routes")
# a single-matrix call's launches by name, the partials its plan needs, gq_debug_route's text for the raw and
# the prepared call, and the workspace size the ABI reports
Route = collections.namedtuple("Route", "names partial raw prepared workspace")


@functools.lru_cache(maxsize=None)
def table():
    """cases: {family: [Case]}; best: {(Kernel, form, N): Call}; selected: every (Kernel, form) any swept call
    launches; routes: {Call: Route} of the single-matrix calls.  The
    library's tuning is reset to the environment's."""
    best, selected, routes = {}, set(), {}
    try:
        for cus in (CUS, SMALL_CUS, TINY_CUS):
            for name, _, points, ks, nrows in VECTORS:
                if cus == TINY_CUS:
                    points = tuple(e for e in points if e in ("ex", "prepared"))
                set_vector(name, cus)
                for call in _calls(name, points, ks, nrows, cus):
                    launches = plan(call)
                    if call.entry in ("ex", "prepared"):
                        (fmt, m, K), t = call.items[0], kl.TYPES[call.items[0][0]]
                        routes[call] = Route(tuple(kl.GEMM_KERNELS[p.kernel] for p in launches),
                                             max([p.partial_bytes for p in launches] or [0]),
                                             kl.route_name(t, m, call.N, K, call.act, False),
                                             kl.route_name(t, m, call.N, K, call.act, True),
                                             kl.workspace_size(t, m, call.N, K, call.act))
                    for p in under_test(launches):
                        key = (kernel_of(p), form_of(p, cus), call.N)
                        if "order2" in key[1]:  # (N * K * 2 > 4 MiB: K = 16640 at 128 tokens, a CPU ideal of
                            key = key[:2] + (0,)  # 0.3-1 s per type -- one token count per form, the smallest K's)
                        selected.add(key[:2])
                        old = best.get(key)
                        if old is None or (call.items[0][2], call.N) < (old.items[0][2], old.N):
                            best[key] = call
    finally:
        kl.reset_tuning()
    covers = collections.defaultdict(list)
    for (kernel, form, N), call in best.items():
        covers[call].append((kernel, form))
    cases = {f: [] for f in FAMILIES}
    for call, cov in covers.items():
        fams = [k.name for k, _ in cov if k.name in FAMILIES]
        family = fams[0] if fams else {"gemm_reduce_f16_kernel": None, "gemm_reduce_kernel": "gemm_kernel",
                                       "reduce_grouped_kernel": "sgemm_grouped_kernel",
                                       "kstream_reduce_kernel": "kstream_kernel"}[cov[0][0].name]
        if family is None:  # (a fp16 split sum kept for itself: beside which kernel does this call launch it?)
            set_vector(call.vector, call.cus)
            family = next(kl.GEMM_KERNELS[p.kernel] for p in plan(call) if kl.GEMM_KERNELS[p.kernel] in FAMILIES)
            kl.reset_tuning()
        cases[family].append(Case(call, family, tuple(sorted(cov))))
    for f in cases:
        cases[f].sort(key=lambda c: (c.covers, c.call))
    return Table(cases, best, selected, routes)


def case_id(c):
    k, form = next(((k, f) for k, f in c.covers if k.name == c.family), c.covers[0])
    fmt, rows, K = c.call.items[0]
    return (f"{k.name.replace('_kernel', '')}{'_'.join(str(a) for a in k.args)}-{fmt}-{'.'.join(form) or 'plain'}-{c.call.act}"
            f"-{c.call.entry}-N{c.call.N}-K{K}-cus{c.call.cus}-{c.call.vector}")


def reached(name):
    """The kernels of a template that some case covers."""
    return {k for cs in table().cases.values() for c in cs for k, _ in c.covers if k.name == name}


# ---- the bit-for-bit identities of a case (tests/test_gpu_gemm_cases.py runs them, the host test counts them) ----
def bits_key(p):
    """What fixes an output's bits besides the inputs: the kernel's arithmetic and its K split.  (ES, the
    in-launch sum, the grid order, sgemm_full_body and where the activations are quantized are claimed not
    to; a stream-K plan also splits by its workgroup count.)"""
    k = kernel_of(p)
    args = k.args[:2] if k.name == "rgemm_kernel" else (k.args[:6] if k.name == "gemm_kernel" else k.args)
    return (k.name, args, p.splits, p.chunks_per_split) + ((p.blocks,) if p.streamk else ())


def main_keys(entries):
    return [bits_key(p) for p in entries if kl.GEMM_KERNELS[p.kernel] in FAMILIES]


def flags(entries):
    return sorted((kl.GEMM_KERNELS[p.kernel], p.es, p.ilc, p.order, p.full) for p in entries
                  if kl.GEMM_KERNELS[p.kernel] in FAMILIES)


def other_cus(call):
    return SMALL_CUS if call.cus == CUS else CUS


def apply(call, **over):
    """The call's tuning vector and GQ_CUS, then the overrides."""
    set_vector(call.vector, over.pop("GQ_CUS", call.cus))
    for k, v in over.items():
        kl.set_tuning(k, v)


def identities(c):
    """(the case's plan entries, [(label, tuning overrides, call)]): the reruns whose output must have the case's
    bits, decided from the plan query alone -- the other side keeps kernel and K split and changes the form.
    Labels: "cus", "GQ_RGEMM_ILC", "GQ_RGEMM_ESTORE", "GQ_SGEMM_FULL", "aq" (the prepared call of a raw one)."""
    call = c.call
    apply(call)
    entries = under_test(plan(call))
    key, out = main_keys(entries), []
    apply(call, GQ_CUS=other_cus(call))
    if main_keys(under_test(plan(call))) == key:
        out.append(("cus", dict(GQ_CUS=other_cus(call)), call))
    t = TUNING[call.vector]
    for knob, value in (("GQ_RGEMM_ILC", 0 if t.get("GQ_RGEMM_ILC", 0) else 1),
                        ("GQ_RGEMM_ESTORE", 0 if any(p.es for p in entries) else 1),
                        ("GQ_SGEMM_FULL", 0 if any(p.full for p in entries) else 1)):
        apply(call, **{knob: value})
        e = under_test(plan(call))
        if main_keys(e) == key and flags(e) != flags(entries):
            out.append((knob, {knob: value}, call))
    if call.entry == "ex" and any(p.aq for p in entries):
        apply(call)
        prep = call._replace(entry="prepared")
        e = under_test(plan(prep))
        assert not any(p.aq for p in e), (c, "the prepared call quantizes in the kernel")
        if main_keys(e) == key:
            out.append(("aq", {}, prep))
    return entries, out
