"""The decode case table (tests/decode_cases.py) against the library's own plans and caps (CPU: the
plan query and the cap query are host-only once GQ_CUS is set).

What is proved here, by asking the plan query at every valid K up to 65536 and every token count the
ABI sends to the decode: every kernel the cap query reports is selected by some call or stands in
decode_cases.UNREACHED, which nothing selects; no accepted plan names a kernel beyond its family's
cap; the grouped launcher accepts exactly what its hand-written case lists are reported to carry;
the expert-indexed plan picks the dense one-token kernel."""
import pytest

import decode_cases as DC
import kernels._lib as kl


@pytest.fixture(scope="module")
def T():
    return DC.table()


@pytest.fixture
def cus256(tune):
    tune(GQ_CUS=DC.CUS)


def _keys(T, family, fmt=None):
    """Every (Kernel) some sweep of the family selected, forced ring forms included."""
    out = set()
    for (fam, st, f, act, N, force), sw in T.sweeps.items():
        if fam == family and (fmt is None or f == fmt):
            out |= {DC.Kernel(fam, s, f, nt, itc, img, fp8) for nt, itc, img, fp8, s in set(sw.values())}
    return out


def test_the_cap_query_counts_the_instantiated_kernels(T):
    """csrc/mmq_decode.hip compiles 355 kernels: these and stream_decode_grouped_kernel's 17 (five case
    sets at three token tiles, the fp8 form at two)."""
    n = {f: len(T.kernels[f]) for f in DC.FAMILIES}
    assert (n["dense"], n["id"], n["id_glu"], n["glu"]) == (122, 56, 56, 104)
    assert n["dense"] + n["id"] + n["id_glu"] + n["glu"] + 17 == 355
    assert n["grouped"] == 301  # the (set, type, tile, chunks, ring, form) cases of those 17


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_every_kernel_is_reached_or_listed(T, family):
    listed = {k for k in DC.UNREACHED if k.family == family}
    have = set(T.kernels[family])
    assert listed <= have, listed - have
    missing = have - DC.reached(family) - listed
    assert not missing, f"no K selects {sorted(missing)}: a case or an UNREACHED entry is missing"
    # the list hides nothing: no sweep, under either forced ring form, selected a listed kernel
    assert not (listed & _keys(T, family)), listed & _keys(T, family)
    assert len(T.cases[family]) >= len(have - listed)


def test_unreached_fp8_four_token_tile_at_every_token_count(cus256):
    """UNREACHED's kernels need the fp8 form at 3+ tokens: no such call takes the decode, at any K."""
    assert {(k.nt, k.fp8) for k in DC.UNREACHED} == {(4, 1)}
    for fmt in sorted({k.fmt for k in DC.UNREACHED}):
        for N in range(3, 9):
            for K in range(256, DC.KMAX + 1, 256):
                assert kl.decode_plan("dense", [(kl.TYPES[fmt], DC.M, K)], N, "fp8") == [], (fmt, N, K)


@pytest.mark.parametrize("family", DC.FAMILIES)
def test_no_accepted_plan_is_beyond_the_cap(T, family):
    have = set(T.kernels[family])
    for k in _keys(T, family):
        cap = kl.decode_cap(family, kl.TYPES[k.fmt], k.nt, bool(k.fp8), k.set)
        assert 0 <= k.itc <= cap, (k, cap)
        assert k in have, k


def test_cases_hold_their_k_range(T, cus256):
    """Each case's two K select its kernel when asked one by one through kernels._lib.decode_plan (the
    GPU tests' reading), in every token group, and the groups' tokens add up to the case's N."""
    for family in DC.FAMILIES:
        for c in T.cases[family]:
            k = c.kernel
            if c.force is not None:
                kl.set_tuning("GQ_DECODE_Q6_IMG", c.force)
            for K in (c.kmin, c.kmax):
                n = DC.ID_PAIRS if family in ("id", "id_glu") else c.N
                ps = [p for p in kl.decode_plan(family, DC.items_of(family, k.set, k.fmt, K), n, DC.act_of(k)) if p.item == 0]
                assert ps and {(p.nt, p.itc, p.img, p.fp8, p.set) for p in ps} == {(k.nt, k.itc, k.img, k.fp8, k.set)}, (c, K)
                assert sum(p.tokens for p in ps) == c.N and all(1 <= p.tokens <= k.nt for p in ps), (c, K)
            kl.set_tuning("GQ_DECODE_Q6_IMG", -1)


def test_one_cu_gives_every_case_row_groups_or_several_tasks(T, tune):
    """Under GQ_CUS = 1 (eight waves) a 37-row matrix gets G > 1 rows per task or more than one task
    per wave, with the kernel unchanged: the geometry tests/test_gpu_decode_cases.py runs second."""
    tune(GQ_CUS=1)
    stash = set()
    for family in DC.FAMILIES:
        for c in T.cases[family]:
            k = c.kernel
            if c.force is not None:
                kl.set_tuning("GQ_DECODE_Q6_IMG", c.force)
            for K in (c.kmin, c.kmax):
                n = DC.ID_PAIRS if family in ("id", "id_glu") else c.N
                ps = [p for p in kl.decode_plan(family, DC.items_of(family, k.set, k.fmt, K), n, DC.act_of(k)) if p.item == 0]
                assert ps, (c, K)
                for p in ps:
                    assert (p.nt, p.itc, p.img, p.fp8, p.set) == (k.nt, k.itc, k.img, k.fp8, k.set), (c, K)
                    assert DC.busy(p), (c, K, p.G, p.ngroups, p.nseg, p.grid)
                    if family in ("id_glu", "glu"):
                        assert p.stash_rows == ((p.G if p.nseg == 1 else 1) + 7) // 8 * 8
                        stash.add((family, p.G > 1))
            kl.set_tuning("GQ_DECODE_Q6_IMG", -1)
    # both GLU families run with a stash of several rows per task and with one of a single row
    assert stash == {(f, g) for f in ("id_glu", "glu") for g in (False, True)}


# ---- the grouped launcher's refusals ----
def _grouped(group, N, act="q8_1"):
    return kl.decode_plan("grouped", [(kl.TYPES[f], M, K) for f, M, K in group], N, act)


def test_grouped_refuses_q4_0_beside_q5k_q3k_q2k(cus256):
    for other in ("q5_k", "q3_k", "q2_k"):
        for N in (1, 2, 3, 4):
            for K0, K in ((32, 256), (4096, 4096)):
                assert _grouped([("q4_0", DC.M, K0), (other, DC.M, K)], N) == [], (other, N)
                assert _grouped([(other, DC.M, K), ("q8_0", 5, 256), ("q4_0", DC.M, K0)], N) == [], (other, N)
            assert len(_grouped([("q4_0", DC.M, 32), ("q6_k", DC.M, 256)], N)) == 2   # (set 4 carries set 0's types)
            assert len(_grouped([(other, DC.M, 256), ("q6_k", DC.M, 256)], N)) == 2


def test_grouped_refuses_fp8_beyond_set_0_and_two_tokens(cus256):
    assert len(_grouped([("q4_k", DC.M, 256), ("q6_k", 5, 256)], 2, "fp8")) == 2
    assert _grouped([("q4_k", DC.M, 256), ("q6_k", 5, 256)], 3, "fp8") == []
    for st in (1, 2, 3, 4):
        for N in (1, 2):
            assert _grouped([("q4_k", DC.M, 256), (DC.SET_ITEM[st][0], 5, 256)], N, "fp8") == [], (st, N)
            assert kl.decode_cap("grouped", kl.GQ_Q4_K, N, True, st) == -1


def test_grouped_one_token_items_stop_at_the_sets_cap(T):
    """A set's one-token kernel carries every type up to kGroupItc[set] cached chunks: beside the
    set's item, a matrix is accepted exactly where its own one-token plan stays within that, and then
    with its own kernel's (chunks, ring form)."""
    refused = 0
    for st in (1, 2, 3, 4):
        fmts = sorted({k.fmt for k in T.kernels["grouped"] if k.set == st})
        assert DC.SET_ITEM[st][0] in fmts
        top = max(kl.decode_cap("grouped", kl.TYPES[f], 1, False, st) for f in fmts)  # kGroupItc[set]
        assert top == {1: 4, 2: 3, 3: 3, 4: 5}[st]  # (mmq_decode.hip kGroupItc: a change there is a change here)
        for fmt in fmts:
            for force in ((None, 0, 1) if fmt == "q6_k" else (None,)):
                solo, grp = T.sweeps["dense", 0, fmt, "q8_1", 1, force], T.sweeps["grouped", st, fmt, "q8_1", 1, force]
                want = {K: key[:4] + (st,) for K, key in solo.items() if key[1] <= top}
                assert grp == want, (st, fmt, force, sorted(set(grp) ^ set(want))[:5])
                refused += len(solo) - len(want)
    assert refused > 0
    # at two and four tokens the lists carry every type's own cap: a set accepts what the dense call takes
    for (fam, st, fmt, act, N, force), grp in T.sweeps.items():
        if fam == "grouped" and N > 1:
            solo = T.sweeps["dense", 0, fmt, act, N, force]
            assert {K: key[:4] for K, key in grp.items()} == {K: key[:4] for K, key in solo.items()}, (st, fmt, act, N)
    for (fam, st, fmt, act, N, force), grp in T.sweeps.items():
        if fam == "grouped" and st == 0:
            assert {K: key[:4] for K, key in grp.items()} == {K: key[:4] for K, key in T.sweeps["dense", 0, fmt, act, N, force].items()}


def test_grouped_types_outside_the_set_have_no_cases(T):
    carried = {0: {"q8_0", "q4_k", "q6_k"}, 1: {"q8_0", "q4_k", "q6_k", "q5_k"}, 2: {"q8_0", "q4_k", "q6_k", "q5_k", "q3_k"},
               3: {"q8_0", "q4_k", "q6_k", "q5_k", "q3_k", "q2_k"}, 4: {"q8_0", "q4_k", "q6_k", "q4_0"}}
    for st in DC.SETS:
        assert {k.fmt for k in T.kernels["grouped"] if k.set == st} == carried[st], st
        for fmt in set(DC.FMTS) - carried[st]:
            for nt in DC.TILES:
                assert kl.decode_cap("grouped", kl.TYPES[fmt], nt, False, st) == -1


# ---- the expert-indexed plan and the dense one-token plan ----
@pytest.mark.parametrize("family", ["id", "id_glu"])
def test_expert_indexed_plan_is_the_dense_one_token_plan(T, family):
    """"A pair's outputs are its one-token launch's bits" needs the same kernel: (itc, img) agree at
    every (type, K), and the expert-indexed entry takes exactly the K the dense one-token call takes."""
    n = 0
    for fmt in DC.FMTS:
        for force in ((None, 0, 1) if fmt == "q6_k" else (None,)):
            solo, ids = T.sweeps["dense", 0, fmt, "q8_1", 1, force], T.sweeps[family, 0, fmt, "q8_1", 1, force]
            if family == "id_glu":  # (the last few K before the LDS limit leave no room for the g stash)
                tail = sorted(set(solo) - set(ids))
                assert len(tail) <= 8 and (not tail or tail[0] > max(ids)), (fmt, force, tail[:5])
                solo = {K: key for K, key in solo.items() if K in ids}
            assert ids == solo, (fmt, force, sorted(set(ids) ^ set(solo))[:5])
            n += len(ids)
    assert n > 3000


def test_queries_refuse_nonsense(cus256):
    assert kl.decode_plan("dense", [(7, 37, 256)], 1) == []              # unknown type
    assert kl.decode_plan("dense", [(kl.GQ_Q4_K, 37, 100)], 1) == []     # K not whole blocks
    assert kl.decode_plan("dense", [(kl.GQ_Q4_K, 37, 256)], 5) == []     # five tokens: not the decode
    assert kl.decode_plan("dense", [(kl.GQ_Q5_K, 37, 256)], 1, "fp8") == []
    assert kl.decode_plan("id", [(kl.GQ_Q4_K, 37, 256)], 65) == []       # kMaxIdPairs
    assert kl.decode_plan("glu", [(kl.GQ_Q4_K, 37, 256)], 5) == []
    assert kl.decode_plan("dense", [(kl.GQ_Q4_K, 37, 256), (kl.GQ_Q4_K, 37, 256)], 1) == []  # one item only
    assert kl.decode_cap("dense", 7, 1) == -1 and kl.decode_cap("dense", kl.GQ_Q4_K, 3) == -1
    assert kl.decode_cap("id", kl.GQ_Q4_K, 2) == -1 and kl.decode_cap("id", kl.GQ_Q4_K, 1, True) == -1
    assert kl.decode_cap("glu", kl.GQ_Q4_K, 1, True) == -1 and kl.decode_cap("dense", kl.GQ_Q5_K, 1, True) == -1
    assert kl.decode_cap("grouped", kl.GQ_Q4_K, 1, False, 5) == -1
    with kl.tuning(GQ_CUS=DC.CUS, GQ_NO_FUSED_DECODE=1):
        assert kl.decode_plan("dense", [(kl.GQ_Q4_K, 37, 256)], 1) == []
        assert kl.decode_plan("glu", [(kl.GQ_Q4_K, 37, 256)], 1) == []
