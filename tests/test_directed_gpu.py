"""The directed pictures (directed_pictures.py) on the device: every result field, every
reconstruction plane and the fused deblocking equal the oracle's, on every path that carries a copy
of the intra code -- and the census of the *device's* results meets the table the oracle's meets
(test_directed_census.py), so a path that avoided a mode would fail even where the comparison passed.

    route        kernels that predict intra (jmhip_abi.hip)
    flow         k_mb_flow (search_mode 0, RDO off, 4x4 transform: the default path)
    ticks        the same under JMH_FLOW=0: k_mb_analyse + k_mb_final per tick
    ffs_t8       search_mode 0 with the 8x8 transform (no dataflow path)
    epzs_*       search_mode 3: k_mb_intra, with transform_8x8_mode 1 also k_mb_intra8
    full_*       search_mode -1, likewise
    rdo_*        the RDO kernels' own loop, CAVLC and CABAC rates
    bits10       the 16-bit instantiations (search_mode 3)
Each with one slice per picture and with slices of 5 macroblocks; the P family with and without
constrained intra prediction.  64x48 pictures, one Encoder per case.
"""
import numpy as np
import pytest

import directed_pictures as dp
import oracle_lib
from jmpaths import ensure_built, load_jmhip
from test_flow_gpu import env
from test_gpu_parity import assert_same

jmhip = load_jmhip()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    ensure_built()
    jmhip.load()


class Route:
    def __init__(self, name, kw, div=1, env=None, flow=False):
        self.name, self.kw, self.div, self.env, self.flow = name, kw, div, env or {}, flow
        self.bit_depth, self.t8 = kw.get("bit_depth", 8), kw.get("transform_8x8_mode", 0)

    def __repr__(self):
        return self.name


ROUTES = [Route(c.name if c.name != "ffs_t4" else "flow", c.kw, c.div, flow=c.name == "ffs_t4") for c in dp.CONFIGS]
ROUTES.insert(1, Route("ticks", ROUTES[0].kw, env=dict(JMH_FLOW=0)))

_sets, _oracle = {}, {}


def sets(bit_depth):
    if bit_depth not in _sets:
        _sets[bit_depth] = (dp.for_depth(dp.intra_sets(), bit_depth), dp.for_depth(dp.p_sets(), bit_depth))
    return _sets[bit_depth]


def oracle(kw, which):
    """The oracle's (results, reconstruction, deblocked picture) of every picture of the I (which 0) or P
    (1) sets under kw: computed once, shared by the routes that differ only on the device."""
    key = (tuple(sorted(kw.items())), which)
    if key not in _oracle:
        bd = kw.get("bit_depth", 8)
        o = oracle_lib.OracleEncoder(dp.W, dp.H, **kw)
        out = []

        def each(s, i, res, rec):
            out.append((res, rec, jmhip.deblock_ref(rec, res, dp.W // 16, dp.H // 16, s.qp, bit_depth=bd)))
        dp.run_sets(o, sets(bd)[which], kw.get("slice_mbs", 0), each)
        o.close()
        for res, rec, dbk in out:
            for a in (res,) + rec + dbk:
                a.setflags(write=False)
        _oracle[key] = out
    return _oracle[key]


def run_case(route, which, tbl, **more):
    kw = dict(search_range=8, **route.kw, **more)
    ref = oracle(kw, which)
    with env(**route.env):
        g = jmhip.Encoder(dp.W, dp.H, **kw)
    c, k = dp.Counter(), 0
    for s in sets(route.bit_depth)[which]:
        for i, pic in enumerate(s.pics):
            if s.refs:
                g.set_reference(*s.refs[i])
            gres, grec = g.encode(*pic, s.slice_type, s.qp, deblock=(0, 0, 0))
            gdbk = g.deblocked()
            ores, orec, odbk = ref[k]
            k += 1
            try:
                assert_same(gres, grec, ores, orec, dp.W // 16)
                for pl, (a, b) in enumerate(zip(gdbk, odbk)):
                    assert np.array_equal(a, b), f"deblocked plane {pl} differs first at (y, x) = {tuple(np.argwhere(a != b)[0])}"
            except BaseException as e:
                raise AssertionError(f"{route.name} {more}: set {s.name} picture {i} (QP {s.qp}): {e}") from e
            c += dp.census(gres, s.slice_type, dp.W, kw.get("slice_mbs", 0))
    t = g.timing()
    g.close()
    assert (t.flow_launches > 0) == route.flow, (route.name, t.flow_launches)
    misses = dp.table_misses(c, tbl)
    assert not misses, "the device's own census misses " + ", ".join(f"{k}: {n} < {v}" for k, n, v in misses)


@pytest.mark.parametrize("slice_mbs", [0, 5])
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_directed_intra(route, slice_mbs):
    run_case(route, 0, dp.table(route.t8, slice_mbs, route.div), slice_mbs=slice_mbs)


@pytest.mark.parametrize("slice_mbs", [0, 5])
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_directed_p(route, slice_mbs):
    """Intra macroblocks between inter ones (unconstrained: they predict from the inter neighbours'
    reconstruction)."""
    run_case(route, 1, dp.p_table(route.t8, 0, route.div), slice_mbs=slice_mbs)


@pytest.mark.parametrize("route", [r for r in ROUTES if r.name != "ticks"], ids=repr)
def test_directed_p_constrained(route):
    """constrained_intra_pred 1: the inter neighbours are not available to the intra macroblocks (there is
    no dataflow path: flow and ticks are one route here)."""
    r = Route(route.name, route.kw, route.div, route.env, flow=False)
    run_case(r, 1, dp.p_table(route.t8, 1, route.div), constrained_intra_pred=1)
