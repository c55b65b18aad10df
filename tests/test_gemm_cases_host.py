"""The GEMM case table (tests/gemm_cases.py) against the library's own symbol table and plans (CPU: the
plan query is host-only once GQ_CUS is set).

What is proved here, by asking the plan query over gemm_cases.VECTORS at GQ_CUS = 256, 8 and (single matrices) 4:
every kernel the library holds is launched by some case or stands in gemm_cases.UNREACHED, which nothing
launches; no accepted plan names an instantiation the library lacks (at run time that would be
hipErrorInvalidValue, or a wrong kernel); gq_debug_route's family agrees with the plan query; the workspace
the ABI reports covers the plan's partials."""
import ctypes

import pytest

import gemm_cases as GC
import kernels._lib as kl


@pytest.fixture(scope="module")
def T():
    return GC.table()


def _all(inv):
    return {k for ks in inv.values() for k in ks}


def test_stub_symbols_parse():
    k = GC.stub_kernel("_ZN2gq12_GLOBAL__N_126__device_stub__gemm_kernelILi0ELi1ELi1ELi0ELi0ELi4ELi1EEEvPKhPKvPKfPtPflllllii")
    assert k == GC.Kernel("gemm_kernel", (0, 1, 1, 0, 0, 4, 1))
    k = GC.stub_kernel("_ZN2gq12_GLOBAL__N_136__device_stub__kstream_reduce_kernelENS0_4KRedE")
    assert k == GC.Kernel("kstream_reduce_kernel", ())
    assert GC.stub_kernel("_ZN2gq10plan_rgemmElll") is None


def test_the_inventory_counts_the_instantiated_kernels():
    """mmq_rgemm.hip 139, mmq_gemm.hip 54, mmq_skinny.hip 22, mmq_kstream.hip 5: a new instantiation fails
    here, and in test_every_kernel_is_reached_or_listed until it has a case."""
    n = {name: len(ks) for name, ks in GC.built_kernels().items()}
    assert (n["rgemm_kernel"], n["sgemm_kernel"], n["sgemm_id_kernel"], n["sgemm_grouped_kernel"],
            n["reduce_grouped_kernel"]) == (63, 28, 28, 16, 4)
    assert (n["gemm_kernel"], n["gemm_reduce_f16_kernel"], n["gemm_reduce_kernel"]) == (41, 8, 5)
    assert n["skinny_kernel"] == 22 and (n["kstream_kernel"], n["kstream_reduce_kernel"]) == (4, 1)
    assert sum(n.values()) == 139 + 54 + 22 + 5
    for ks in GC.built_kernels().values():
        assert len(set(ks)) == len(ks)


@pytest.mark.parametrize("name", GC.FAMILIES + GC.REDUCES)
def test_every_kernel_is_reached_or_listed(T, name):
    have = set(GC.built_kernels()[name])
    listed = {k for k in GC.UNREACHED if k.name == name}
    assert listed <= have, listed - have
    got = GC.reached(name)
    assert got <= have, f"the table names kernels the library lacks: {sorted(got - have)}"
    assert got | listed == have, f"no case launches {sorted(have - got - listed)}: a case or an UNREACHED entry is missing"
    # the list hides nothing: no swept call, under any vector at either GQ_CUS, launches a listed kernel
    assert not (listed & {k for k, _ in T.selected})
    assert not (listed & got)


def test_unreached_is_the_loaderless_and_the_64_token_aq_forms():
    assert len(GC.UNREACHED) == 17 and len(set(GC.UNREACHED)) == 17
    for k in GC.UNREACHED:
        f, nb, rg, abl, am, nl, aq = k.args
        assert k.name == "gemm_kernel" and am == 0 and abl == 0
        assert (nl, aq) == (0, 0) and rg == 1 or (nb, rg, nl, aq) == (8, 2, 4, 0) or (nb, rg, nl, aq) == (4, 1, 4, 1), k


def test_no_accepted_plan_names_a_kernel_the_library_lacks(T):
    have = _all(GC.built_kernels())
    sel = {k for k, _ in T.selected}
    assert sel <= have, sorted(sel - have)
    assert len(T.selected) > 300  # (kernel, form) pairs: the sweep saw the forms, not one call per kernel


def test_every_form_has_a_case(T):
    covered = {kf for cs in T.cases.values() for c in cs for kf in c.covers}
    assert covered == T.selected
    for family, cs in T.cases.items():
        assert cs and all(c.family == family for c in cs)
        assert len({c.call for c in cs}) == len(cs)


def test_the_forms_the_kernels_branch_into_are_in_the_table(T):
    forms = {}
    for k, f in T.selected:
        forms.setdefault(k.name, set()).add(f)
    assert {("whole",), ("split",), ("split", "ilc"), ("split", "rounds"), ("split", "rounds", "chipfull")} <= forms["rgemm_kernel"]
    assert ("whole", "order0", "chipfull") in forms["sgemm_kernel"] and ("whole", "chipfull") in forms["gemm_kernel"]
    sg = forms["sgemm_kernel"]
    assert {f[1] for f in sg} == {"order0", "order1", "order2"} and any("full" in f for f in sg) and any("rounds" in f for f in sg)
    assert {("whole",), ("split", "pf16"), ("split", "pf32")} <= forms["gemm_kernel"]
    assert forms["sgemm_id_kernel"] == {(), ("full",)}
    assert {f[0] for f in forms["kstream_kernel"]} == {"aq0", "aq1", "aq2"}
    gr = forms["sgemm_grouped_kernel"]
    assert {f[0] for f in gr} == set(GC.FMTS) and any("streamk" in f and "ilc" in f for f in gr) and any("full" in f for f in gr)
    # the split-major order needs N*K*2 > 4 MiB and blocks % 8 == 0: 128 tokens from K = 16640
    o2 = [c for (k, f, N), c in T.best.items() if k.name == "sgemm_kernel" and "order2" in f]
    assert o2 and all(c.N * c.items[0][2] * 2 > 4 << 20 for c in o2) and min(c.items[0][2] for c in o2) == 16640
    # kstream: two super-blocks per wave from K = 2304, two K ranges and their sum from 4352
    assert min(c.items[0][2] for (k, f, N), c in T.best.items() if k == GC.Kernel("kstream_kernel", (1, 2))) == 2304
    assert min(c.items[0][2] for (k, f, N), c in T.best.items() if k.name == "kstream_reduce_kernel") == 4352


def _first_and_rest(route):
    """A gq_debug_route text as the launches it names: (first kernel, the exact tuple or None when the text
    lists a reduce whether or not the plan splits)."""
    if route in ("none", "stream_decode_kernel", "gemv_kernel", "dequant_kernel + hipBLASLt"):
        return None, ()
    names = tuple(w for w in route.replace("(", " ").replace(")", " ").split() if w.endswith("_kernel"))
    exact = names if names[0] in ("rgemm_kernel", "sgemm_kernel", "kstream_kernel", "skinny_kernel") else None
    return names[0], exact


def test_route_names_agree_with_the_plan_query(T):
    """gq_debug_route's family is the plan query's first kernel for every swept single-matrix call; for the
    kernels whose route text says whether a reduce follows, the whole launch list agrees.  A raw call
    (gq_mmq_ex) that is not one launch on the caller's activations runs act_quant and the prepared call's
    plan: the query reports that one, gq_debug_route(prepared = 0) the raw plan's."""
    assert len(T.routes) > 50000
    raw_differs = 0
    for call, r in T.routes.items():
        got = r.names[0] if r.names else None
        first, exact = _first_and_rest(r.prepared)
        if call.entry == "ex" and got != first:
            first, exact = _first_and_rest(r.raw)
            raw_differs += 1
        assert got == first, (call, r)
        if exact is not None:
            assert r.names == exact, (call, r)
    assert raw_differs > 0


def _act_bytes(act, N, K):
    """The activation part of the workspace at GEMM token counts (gq_capi.hip carve), without the decode
    token counts' fp16 copy: a lower bound."""
    al = lambda v: (v + 255) & ~255
    if act == "fp8":
        return al(N * K * 2)
    sc = (K // 32) * ((N + 3) & ~3) * 4
    return al(N * K * 2) + al(N * K) + 2 * al(sc) if N > 4 else 0


def test_the_reported_workspace_covers_the_plans_partials(T):
    n = 0
    for call, r in T.routes.items():
        if r.partial:
            fmt, rows, K = call.items[0]
            assert r.workspace >= _act_bytes(call.act, call.N, K) + r.partial, (call, r)
            n += 1
    assert n > 10000


def test_grouped_and_sorted_workspaces_cover_their_plans(T, tune):
    fake = 4096  # (the size queries compute addresses from the pointers and read nothing)
    n = 0
    for cs in (T.cases["sgemm_grouped_kernel"], T.cases["kstream_kernel"], T.cases["sgemm_id_kernel"]):
        for c in cs:
            call = c.call
            GC.set_vector(call.vector, call.cus)
            entries = GC.plan(call)
            if call.entry == "grouped_prepared":
                arr = (kl.GemmItem * len(call.items))(*[kl.GemmItem(kl.TYPES[f], fake, fake, fake, m, m, k) for f, m, k in call.items])
                size = kl.lib().gq_mmq_grouped_prepared_workspace_size(kl.ACTS[call.act], arr, len(call.items), call.N)
                ks = sum(p.partial_bytes for p in entries if kl.GEMM_KERNELS[p.kernel] == "kstream_kernel")
                gr = max([p.partial_bytes for p in entries if kl.GEMM_KERNELS[p.kernel] == "sgemm_grouped_kernel"] or [0])
                assert size >= ks + gr, (call, size, ks, gr)
                n += 1
            elif call.entry == "id_sorted":
                fmt, rows, K = call.items[0]
                size = kl.lib().gq_mmq_id_sorted_workspace_size(kl.TYPES[fmt], GC.E, rows, call.N, GC.S, K)
                assert size >= call.N * GC.S * (K * 2 + 4) + 16 + 16 * entries[0].tiles_n, (call, size)
                n += 1
    assert n > 500


def test_cases_hold_their_plans(T, tune):
    """Each case's call, asked one by one through kernels._lib.gemm_plan (the GPU tests' reading), launches the
    (kernel, form) pairs it is kept for."""
    for cs in T.cases.values():
        for c in cs:
            GC.set_vector(c.call.vector, c.call.cus)
            got = {(GC.kernel_of(p), GC.form_of(p, c.call.cus)) for p in GC.under_test(GC.plan(c.call))}
            assert set(c.covers) <= got, (c, got)


def test_the_small_chips_reach_the_branches_a_whole_chip_never_takes(T, tune):
    """Grids of several rounds and persistent kernels whose workgroups take several units show up at these
    shapes only when the plan is made for SMALL_CUS; the planners' `tiles >= cus` branch -- one split by the
    auto rule -- only for TINY_CUS, where a 2 x 2 or 3 x 2 tile grid covers the planned chip."""
    small = {(k.name, f) for (k, f, N), c in T.best.items() if c.cus != GC.CUS}
    names = {n for n, f in small if "rounds" in f}
    assert {"rgemm_kernel", "sgemm_kernel", "gemm_kernel", "skinny_kernel", "kstream_kernel"} <= names
    assert not any("rounds" in f or "chipfull" in f for (k, f, N), c in T.best.items() if c.cus == GC.CUS)
    assert not any("chipfull" in f for (k, f, N), c in T.best.items() if c.cus == GC.SMALL_CUS)
    # tiles >= cus with the splits left to the planner: plan_sgemm and plan_gemm answer one split, a whole
    # launch on a grid as large as the planned chip; plan_rgemm splits per super-block whatever the chip
    auto = {"sgemm_kernel": [], "gemm_kernel": [], "rgemm_kernel": []}
    for cs in T.cases.values():
        for c in cs:
            t = GC.TUNING[c.call.vector]
            if c.call.cus != GC.TINY_CUS or t.get("GQ_SGEMM_SPLITS", 0) or t.get("GQ_GEMM_SPLITS", 0):
                continue
            GC.set_vector(c.call.vector, c.call.cus)
            for p in GC.under_test(GC.plan(c.call)):
                name = kl.GEMM_KERNELS[p.kernel]
                if name in auto and p.tiles_m * p.tiles_n >= GC.TINY_CUS and (GC.kernel_of(p), GC.form_of(p, GC.TINY_CUS)) in c.covers:
                    auto[name].append(p.splits)
                    assert "chipfull" in GC.form_of(p, GC.TINY_CUS)
    assert auto["sgemm_kernel"] and set(auto["sgemm_kernel"]) == {1}, auto["sgemm_kernel"]
    assert auto["gemm_kernel"] and set(auto["gemm_kernel"]) == {1}, auto["gemm_kernel"]
    assert auto["rgemm_kernel"]


def test_every_identity_has_pairs_in_every_family_it_applies_to(T, tune):
    """tests/test_gpu_gemm_cases.py compares bits only where the plan query says the other side keeps kernel and K
    split (gemm_cases.identities).  A planning change that made a comparison vanish would pass there unseen: here
    each identity is counted per family, and sgemm_kernel's three grid orders are all paired through GQ_RGEMM_ILC."""
    n = {}
    orders = set()
    for family, cs in T.cases.items():
        if family == "sgemm_id_kernel":
            continue
        for c in cs:
            entries, same = GC.identities(c)
            for label, over, call in same:
                n[family, label] = n.get((family, label), 0) + 1
                if family == "sgemm_kernel" and label == "GQ_RGEMM_ILC":
                    GC.apply(call, **dict(over))
                    orders.add((entries[0].order, GC.under_test(GC.plan(call))[0].order))
    want = {"rgemm_kernel": ("cus", "GQ_RGEMM_ILC", "GQ_RGEMM_ESTORE", "aq"), "sgemm_kernel": ("cus", "GQ_RGEMM_ILC", "GQ_SGEMM_FULL"),
            "sgemm_grouped_kernel": ("cus", "GQ_RGEMM_ILC", "GQ_SGEMM_FULL"), "gemm_kernel": ("cus", "aq"),
            "skinny_kernel": ("cus",), "kstream_kernel": ("cus", "aq")}
    for family, labels in want.items():
        for label in labels:
            assert n.get((family, label), 0) >= 10, (family, label, n)
        assert n[family, "cus"] * 10 >= 8 * len(T.cases[family]), (family, n[family, "cus"], len(T.cases[family]))
    assert {(0, 1), (1, 0), (2, 1)} <= orders, orders
    # the sorted GEMM's whole-super-block form against the plain one: both are cases of the same kernels
    full = {k for k, f in T.selected if k.name == "sgemm_id_kernel" and f == ("full",)}
    assert full and full <= {k for k, f in T.selected if k.name == "sgemm_id_kernel" and f == ()}


def test_query_refuses_nonsense(tune):
    tune(GQ_CUS=GC.CUS)
    assert kl.gemm_plan("ex", [(7, 293, 256)], 16) == []                # unknown type
    assert kl.gemm_plan("ex", [(kl.GQ_Q4_K, 293, 100)], 16) == []       # K not whole blocks
    assert kl.gemm_plan("ex", [(kl.GQ_Q4_K, 293, 256)], 1) == []        # the decode: no GEMM kernel
    assert kl.gemm_plan("prepared", [(kl.GQ_Q4_K, 293, 256)], 768) == []  # the library GEMM
    assert kl.gemm_plan("ex", [(kl.GQ_Q4_K, 293, 256), (kl.GQ_Q4_K, 293, 256)], 16) == []  # one item only
    assert kl.gemm_plan("grouped_ex", [(kl.GQ_Q4_K, 304, 256)], 4) == []  # the grouped decode's tokens
    assert kl.gemm_plan("grouped_ex", [(kl.GQ_Q4_K, 293, 256)], 16) == []  # M % 16 != 0: not the stream
    assert kl.gemm_plan("grouped_ex", [(kl.GQ_Q5_K, 304, 256)], 16) == []
    assert kl.gemm_plan("grouped_prepared", [(kl.GQ_Q4_0, 293, 256), (kl.GQ_Q3_K, 5, 256)], 16) == []  # sets 3 and 1
    assert kl.gemm_plan("id_sorted", [(kl.GQ_Q4_K, 293, 256)], 16, E=0, S=2) == []
    assert kl.lib().gq_debug_gemm_plan(9, 0, (kl.GroupItem * 1)(kl.GroupItem(1, None, None, 256, None, 293, 293, 256)), 1, 16, 0, 0,
                                       (kl.GemmPlan * 1)(), 1) == 0
    assert ctypes.sizeof(kl.GemmPlan) == 112
