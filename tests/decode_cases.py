"""The case table of the streaming decode (csrc/mmq_decode.hip), built from the library itself.

The cap query (gq_debug_decode_cap) says which kernels each family has: decode_body<F, NT, ITC, IM,
FP8, GLU> as stream_decode_kernel ("dense"), stream_decode_id_kernel ("id"),
stream_decode_id_glu_kernel ("id_glu"), stream_decode_glu_kernel ("glu") and the cases of
stream_decode_grouped_kernel<NT, FP8, SET> ("grouped").  The plan query (gq_debug_decode_plan) says
which kernel a call takes.  table() asks the plan query at every valid K up to 65536 -- host only,
GQ_CUS = 256 -- and keeps, per kernel and token count, the smallest and the largest K that select
it: tests/test_decode_cases_host.py proves from it that every kernel is reached or listed in
UNREACHED, tests/test_gpu_decode_cases.py runs every case.

A new decode family or block type belongs here (FAMILIES, FMTS, SET_ITEM) before it is done."""
import collections
import functools

import kernels._lib as kl

M = 37          # rows of every case: odd, a ragged last row group
KMAX = 65536
CUS = 256       # the chip the table is planned for (nt, itc, img never depend on it)
FAMILIES = ("dense", "id", "id_glu", "glu", "grouped")
FMTS = ("q8_0", "q4_k", "q6_k", "q5_k", "q3_k", "q2_k", "q4_0")
TILES = (1, 2, 4)
TOKENS = {"q8_1": (1, 2, 3, 4), "fp8": (1, 2)}   # the token counts the ABI sends to the decode
ID_PAIRS = 4    # the expert-indexed cases: N = 2 tokens x S = 2 slots
SETS = (0, 1, 2, 3, 4)
# a grouped launch's second item: the smallest matrix of the type that defines the case set
# (FmtInfo::group_set; set 0 has no such type: Q4_K)
SET_ITEM = {0: ("q4_k", 5, 256), 1: ("q5_k", 5, 256), 2: ("q3_k", 5, 256), 3: ("q2_k", 5, 256), 4: ("q4_0", 5, 32)}

# family, case set (grouped; else 0), type name, token tile, cached chunks, Q6_K ring image, fp8 form
Kernel = collections.namedtuple("Kernel", "family set fmt nt itc img fp8")
# force: the GQ_DECODE_Q6_IMG value the case needs (None: the default rule picks kernel.img)
Case = collections.namedtuple("Case", "kernel N force kmin kmax")

# Kernels that exist (the cap query) and that no call reaches, whatever K: the fp8 form at a four-token
# tile.  walk<DensePolicy> instantiates it with the other tiles, and the ABI sends the fp8 variant to
# the decode at one and two tokens only (gq_capi.hip plan_call).  test_decode_cases_host.py asserts
# by the exhaustive search that nothing reaches them.  ("The decode case table".)
UNREACHED = [Kernel("dense", 0, fmt, 4, 0, img, 1) for fmt, img in (("q8_0", 0), ("q4_k", 0), ("q6_k", 0), ("q6_k", 1))]


def act_of(kernel):
    return "fp8" if kernel.fp8 else "q8_1"


def case_id(c):
    k = c.kernel
    return (f"{k.family}{k.set if k.family == 'grouped' else ''}-{k.fmt}-nt{k.nt}-itc{k.itc}-img{k.img}"
            f"{'-fp8' if k.fp8 else ''}-N{c.N}")


def kernels(family):
    """Every kernel the cap query reports for the family."""
    out = []
    for st in (SETS if family == "grouped" else (0,)):
        for fmt in FMTS:
            for fp8 in (0, 1):
                for nt in TILES:
                    cap = kl.decode_cap(family, kl.TYPES[fmt], nt, bool(fp8), st)
                    for itc in range(cap + 1):
                        out += [Kernel(family, st, fmt, nt, itc, img, fp8) for img in ((0, 1) if fmt == "q6_k" else (0,))]
    return out


def items_of(family, st, fmt, K):
    """The (type, M, K) list of a case's call: the matrix under test, in a grouped launch beside SET_ITEM."""
    head = [(kl.TYPES[fmt], M, K)]
    if family != "grouped":
        return head
    f2, m2, k2 = SET_ITEM[st]
    return head + [(kl.TYPES[f2], m2, k2)]


def busy(p):
    """A plan entry (kl.DecodePlan) whose waves take several rows per task (G > 1) or more than one task
    each -- ring slots reused -- which a 37-row matrix on a whole chip never does."""
    return p.G > 1 or p.ngroups * p.nseg > p.grid * 8


def _sweep(family, st, fmt, act, N):
    """{K: (nt, itc, img, fp8, set)} over every K the family's entry takes on its one-launch decode, for
    the matrix under test (item 0) under the current tuning.  set: the case set of the launch that
    holds it -- a Q6_K item of K >= 8192 at 3-4 tokens runs at a two-token tile, in a launch without
    the four-token SET_ITEM, hence of set 0."""
    L = kl.lib()
    fid, aid = kl.DECODE_FAMILIES[family], kl.ACTS[act]
    its = items_of(family, st, fmt, 0)
    arr = (kl.GroupItem * len(its))(*[kl.GroupItem(t, None, None, k, None, m, m, k) for t, m, k in its])
    out = (kl.DecodePlan * 16)()
    qk = kl.BLOCK_ELEMS[kl.TYPES[fmt]]
    n = ID_PAIRS if family in ("id", "id_glu") else N
    got = {}
    for K in range(qk, KMAX + 1, qk):
        arr[0].K = arr[0].ldb = K
        cnt = L.gq_debug_decode_plan(fid, aid, arr, len(its), n, out, 16)
        for p in out[:min(cnt, 16)]:
            if p.item == 0:
                assert not p.lds_split, (family, fmt, K)
                got[K] = (p.nt, p.itc, p.img, p.fp8, p.set)
                break
    return got


Table = collections.namedtuple("Table", "cases sweeps kernels")


@functools.lru_cache(maxsize=None)
def table():
    """cases: {family: [Case]}; sweeps: {(family, set, fmt, act, N, force): {K: (nt, itc, img, fp8, set)}};
    kernels: {family: [Kernel]}.  The library's tuning is left as it was found."""
    sweeps, cases, kern = {}, {}, {}
    with kl.tuning(GQ_CUS=CUS):
        for family in FAMILIES:
            kern[family] = kernels(family)
            for st in (SETS if family == "grouped" else (0,)):
                for fmt in FMTS:
                    for act in ("q8_1", "fp8"):
                        # (no kernel of the type and form, e.g. a type the set's kernel does not carry: no sweep;
                        # test_decode_cases_host.py asserts the refusals)
                        if not any(k.set == st and k.fmt == fmt and act_of(k) == act for k in kern[family]):
                            continue
                        for N in ((1,) if family in ("id", "id_glu") else TOKENS[act]):
                            for force in ((None, 0, 1) if fmt == "q6_k" else (None,)):
                                if force is not None:
                                    kl.set_tuning("GQ_DECODE_Q6_IMG", force)
                                sweeps[family, st, fmt, act, N, force] = _sweep(family, st, fmt, act, N)
                                kl.set_tuning("GQ_DECODE_Q6_IMG", -1)
            cases[family] = []
            for k in kern[family]:
                act = act_of(k)
                for N in ((1,) if family in ("id", "id_glu") else TOKENS[act]):
                    for force in ((None, k.img) if k.fmt == "q6_k" else (None,)):
                        sw = sweeps.get((family, k.set, k.fmt, act, N, force), {})
                        ks = [K for K, key in sw.items() if key == (k.nt, k.itc, k.img, k.fp8, k.set)]
                        if ks:
                            cases[family].append(Case(k, N, force, min(ks), max(ks)))
                            break
    return Table(cases, sweeps, kern)


def reached(family):
    return {c.kernel for c in table().cases[family]}
