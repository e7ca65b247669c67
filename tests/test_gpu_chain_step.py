"""GPU parity: the Golub-Kahan step of a FORWARD chain L = R o A o P in one pass (jh_chain_bidiag_step; k_chain_adj MODE 2, jh_tall_chain_step.hip).

The step is the composed sequence the solvers run over vec(L) (src/Jets.jl:1138-1154): the FORWARD chain into a temporary (530-540), `u .= alpha*tmp
.+ beta*u`, ||u||^2, and the ADJOINT chain of L' -- so the bar is that sequence's BITS for u and w (the planner's chains on the device, and the same
stages applied one by one with chains.ENABLED = False), ||u||^2 to fp64 round-off, the oracle's stage-by-stage rows at the headline size, and
tolerance where the many-small-rows split walk sums w in parts."""
import numpy as np
import pytest

from .helpers import DTYPES, assert_bits_equal, u01
from .test_gpu_chains import Rig

pytestmark = pytest.mark.gpu

STEP_CHAINS = {
    # name: tokens in application order (tests/test_gpu_chains.py: Rig)
    "W o A": ["A", ("W", 0, False)],
    "Wb o A": ["A", ("Wb", 0, False)],
    "W o A o M": [("M", 0, False), "A", ("W", 0, False)],
    "0.75 * (W o A)": ["A", ("W", 0, False), ("s", 0.75, "r")],
    "W2 o W1 o A": ["A", ("W", 0, False), ("W", 1, True)],
}


def _composed(J, L, u0, v, alpha, beta):
    """FORWARD chain -> lincomb -> ADJOINT chain of L', as the solver loops compose them."""
    tmp = J.mul_(J.zeros(J.range(L)), L, v)
    u = J.copyto_(J.zeros(J.range(L)), u0)
    if beta != 0.0:
        J.lincomb_(u, [alpha, beta], [tmp, u])
    else:
        J.lincomb_(u, [alpha], [tmp])
    w = J.mul_(J.zeros(J.domain(L)), L.H, u)
    return u, w


def _flat(x):
    return x.to_numpy().ravel(order="F")


def _normsq64(x):
    a = _flat(x)
    return float(np.sum(np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2))


def _step(J, sc, L, u0, v, alpha, beta):
    u = J.copyto_(J.zeros(J.range(L)), u0)
    w = J.rand(J.domain(L), seed=55, stream=3)                                   # a dirty output: the step overwrites w
    nsq = sc.step(u, v, w, alpha, beta)
    assert nsq is not None, "the library declined the step"
    return u, w, nsq


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(STEP_CHAINS))
@pytest.mark.parametrize("nrow,n,kinds", [(5, 4096 + 64, "diag"), (7, 1027, "diag"), (18, 2051, "mixed"), (6, 67, "mixed")])
@pytest.mark.parametrize("beta", [0.0, -0.625])
def test_chain_step_has_the_bits_of_the_composed_sequence(Jets, oracle, dt, name, nrow, n, kinds, beta):
    from jets_jl_amd import chains

    J = Jets
    rig = Rig(J, oracle, dt, nrow, n, kinds)
    L = rig.compose(STEP_CHAINS[name])
    sc = chains.SolverChains(L)
    assert sc.fwd is not None, f"{name}: not one FORWARD run"
    v = J.from_numpy(u01(oracle, dt, 93, 0, n), J.domain(L))
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, 94, i, n) for i in range(nrow)]), J.range(L))
    alpha = 1.375
    J.tune(adj_split=0)
    try:
        before = chains.STATS["chain_step_calls"]
        u, w, nsq = _step(J, sc, L, u0, v, alpha, beta)
        assert chains.STATS["chain_step_calls"] == before + 1
        ur, wr = _composed(J, L, u0, v, alpha, beta)
        assert_bits_equal(_flat(u), _flat(ur), f"{name}: u vs the composed sequence")
        assert_bits_equal(_flat(w), _flat(wr), f"{name}: w vs the composed sequence")
        chains.ENABLED[0] = False
        try:
            us, ws = _composed(J, L, u0, v, alpha, beta)
        finally:
            chains.ENABLED[0] = True
        assert_bits_equal(_flat(u), _flat(us), f"{name}: u vs stage by stage")
        assert_bits_equal(_flat(w), _flat(ws), f"{name}: w vs stage by stage")
        want = _normsq64(u)
        assert abs(nsq - want) <= 1e-12 * want, f"{name}: ||u||^2 {nsq} vs {want}"
    finally:
        J.tune(adj_split=-1)
        sc.close()
        rig.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("knobs", [dict(adj_wg=256), dict(adj_wg=512), dict(adj_wg=512, adj_unroll=4), dict(nt=0), dict(nt=2), dict(ua_nt=1)])
def test_every_launch_shape_and_nt_setting(Jets, oracle, dt, knobs):
    """Every shape the step's launcher can pick -- 256 x 1 x 2, 512 x 2 x 1 and 512 x 4 x 1, which ComplexF32 takes as 512 x 2 x 1 (its grid sized
    for that shape) -- and every nontemporal setting, forced once each, in every element type: the bits of the composed sequence."""
    from jets_jl_amd import chains

    J = Jets
    rig = Rig(J, oracle, dt, 9, 3 * 4096 + 17, "mixed")
    L = rig.compose(["A", ("W", 0, False), ("W", 1, True)])
    sc = chains.SolverChains(L)
    n = rig.n
    v = J.from_numpy(u01(oracle, dt, 95, 0, n), J.domain(L))
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, 96, i, n) for i in range(rig.nrow)]), J.range(L))
    saved = {k: J.tune_get(k) for k in list(knobs) + ["adj_unroll", "adj_split"]}
    J.tune(adj_split=0, **knobs)
    try:
        u, w, nsq = _step(J, sc, L, u0, v, -0.5, 2.0)
        ur, wr = _composed(J, L, u0, v, -0.5, 2.0)
        assert_bits_equal(_flat(u), _flat(ur), f"{knobs}: u")
        assert_bits_equal(_flat(w), _flat(wr), f"{knobs}: w")
        want = _normsq64(u)
        assert abs(nsq - want) <= 1e-12 * want
    finally:
        J.tune(**saved)
        sc.close()
        rig.close()


@pytest.mark.parametrize("dt", [np.float32, np.complex64])
def test_split_walk_of_many_small_rows(Jets, oracle, dt):
    """512 rows of small blocks: w's row sum is cut into parts (tolerance against the ordered sum); u is updated row by row either way (bits), and with
    adj_split = 0 the ordered walk gives w's bits."""
    from jets_jl_amd import chains
    from .helpers import rel_err

    J = Jets
    rig = Rig(J, oracle, dt, 512, 1024, "mixed", with_wb=False)
    L = rig.compose(["A", ("W", 0, False), ("s", 0.75, "r")])
    sc = chains.SolverChains(L)
    n = rig.n
    v = J.from_numpy(u01(oracle, dt, 97, 0, n), J.domain(L))
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, 98, i, n) for i in range(rig.nrow)]), J.range(L))
    try:
        J.tune(adj_split=-1)
        u, w, nsq = _step(J, sc, L, u0, v, 1.0, -0.25)
        assert J.tune_get("last_adj_parts") > 1, "this shape should take the split walk"
        J.tune(adj_split=0)
        ur, wr = _composed(J, L, u0, v, 1.0, -0.25)
        assert_bits_equal(_flat(u), _flat(ur), "u (split walk)")
        assert rel_err(_flat(w), _flat(wr)) < (2e-5 if dt == np.float32 or dt == np.complex64 else 1e-13)
        u2, w2, _ = _step(J, sc, L, u0, v, 1.0, -0.25)
        assert_bits_equal(_flat(w2), _flat(wr), "w (ordered walk)")
        want = _normsq64(u)
        assert abs(nsq - want) <= 1e-12 * want
    finally:
        J.tune(adj_split=-1)
        sc.close()
        rig.close()


@pytest.mark.parametrize("dt", [np.complex64, np.float32])
def test_long_rows_take_the_fat_shape_by_default(Jets, oracle, dt):
    """Rows of 128^3 elements (ComplexF32: 1 M packs, enough workgroups for every CU at 2048 packs each): the launcher's own rule picks the fat
    shape -- 512 x 4 x 1, capped to 512 x 2 x 1 for ComplexF32 --, and every element of u and w is the composed sequence's."""
    from jets_jl_amd import chains

    J = Jets
    n = 128 ** 3
    rig = Rig(J, oracle, dt, 3, n, "diag", with_wb=False)
    L = rig.compose(["A", ("W", 0, False)])
    sc = chains.SolverChains(L)
    v = J.from_numpy(u01(oracle, dt, 101, 0, n), J.domain(L))
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, 102, i, n) for i in range(rig.nrow)]), J.range(L))
    J.tune(adj_split=0)
    try:
        u, w, nsq = _step(J, sc, L, u0, v, 0.5, -1.5)
        ur, wr = _composed(J, L, u0, v, 0.5, -1.5)
        assert_bits_equal(_flat(u), _flat(ur), "u")
        assert_bits_equal(_flat(w), _flat(wr), "w")
        want = _normsq64(u)
        assert abs(nsq - want) <= 1e-12 * want
    finally:
        J.tune(adj_split=-1)
        sc.close()
        rig.close()


def test_declined_shapes_keep_their_route(Jets, oracle):
    """R with three range-side stages: R + R^H exceed one list -- the step declines before touching anything (JH_ERR_UNSUPPORTED), u stays."""
    from jets_jl_amd import chains

    J = Jets
    dt = np.float32
    rig = Rig(J, oracle, dt, 5, 1024, "diag")
    L = rig.compose(["A", ("W", 0, False), ("s", 2.0, "r"), ("W", 1, False)])
    sc = chains.SolverChains(L)
    assert sc.fwd is not None
    u0 = J.from_numpy(np.concatenate([u01(oracle, dt, 99, i, 1024) for i in range(5)]), J.range(L))
    u = J.copyto_(J.zeros(J.range(L)), u0)
    v = J.from_numpy(u01(oracle, dt, 100, 0, 1024), J.domain(L))
    assert sc.step(u, v, J.zeros(J.domain(L)), 1.0, 0.5) is None
    assert_bits_equal(_flat(u), _flat(u0), "a declined step leaves u alone")
    sc.close()
    rig.close()


def test_full_size_weighted_step(Jets, oracle):
    """256 x 256^3 Float32 with range weights: the step against the composed sequence, bit for bit -- every element of w and four whole rows of u
    (all of u would be 16 GiB on the host) --, and on sampled slices against the oracle's stage-by-stage rows (jo.block_df / child_mul / block_df_adj)."""
    from jets_jl_amd import chains
    from oracle import jets_oracle as jo

    J = Jets
    dt, nrow, shape = np.float32, 256, (256, 256, 256)
    n = int(np.prod(shape))
    spc = J.JetSpace(dt, *shape)
    A = J.blockop([[J.JopDiagonal(J.rand(spc, seed=1, stream=i))] for i in range(nrow)])
    w8 = J.rand(J.range(A), seed=2, stream=0)
    L = J.JopDiagonal(w8) @ A
    v = J.rand(J.domain(A), seed=3, stream=0)
    sc = chains.SolverChains(L)
    try:
        assert sc.fwd is not None
        u = J.zeros(J.range(A))
        w = J.zeros(J.domain(A))
        nsq = sc.step(u, v, w, 1.0, 0.0)
        got_w = _flat(w)
        J.tune(adj_split=0)
        try:
            ur, wr = _composed(J, L, u, v, 1.0, 0.0)                               # (beta == 0: u0 is not read)
        finally:
            J.tune(adj_split=-1)
        for i in (0, 1, 128, nrow - 1):
            assert_bits_equal(u.arrays[i].to_numpy().ravel(order="F"), ur.arrays[i].to_numpy().ravel(order="F"), f"u row {i} vs the composed sequence")
        assert_bits_equal(got_w, _flat(wr), "w vs the composed sequence")
        del ur, wr
        for s0 in (0, n // 2 + 4096, n - 64):
            k = 64
            hv = jo.rng_u01(dt, 3, 0, s0, k)
            acc = np.zeros(k, dtype=dt)
            for i in range(0, nrow):
                a = jo.rng_u01(dt, 1, i, s0, k)
                wi = jo.rng_u01(dt, 2, 0, i * n + s0, k)
                t = jo.block_df([[jo.Block("diag", k, coeff=a)]], [np.zeros(k, dtype=dt)], [hv])[0]
                t = jo.child_mul(jo.Block("diag", k, coeff=wi), np.zeros(k, dtype=dt), t)            # u_i = W A v (alpha 1, beta 0)
                if i in (0, 77, nrow - 1):
                    got_u = u.arrays[i].to_numpy().ravel(order="F")[s0:s0 + k]
                    assert_bits_equal(got_u, t, f"u row {i} slice at {s0} vs the oracle")
                t = jo.child_mul(jo.Block("diag", k, coeff=wi, adjoint=True), np.zeros(k, dtype=dt), t)  # W'
                acc = acc + jo.block_df_adj([[jo.Block("diag", k, coeff=a)]], [np.zeros(k, dtype=dt)], [t])[0]
            assert_bits_equal(got_w[s0:s0 + k], acc, f"w slice at {s0} vs the oracle")
        assert nsq > 0
        del u, w
    finally:
        sc.close()
        J.close(A)
