"""GPU tests of the table of force families (csrc/families.hip, csrc/amm_ctx.h: ForceFamily): one typed lookup for the eight families,
one release, one dispatch.

An id of family F given to an entry point of family G is refused with G's wording followed by F's noun phrase, tag and entry-point
prefix -- for every ordered pair (F, G) -- and the refused call changes nothing.  A released id is refused by its own family with
the bare wording, by amm_force_eval as a released id, and no group lists it any more.  amm_set_slice refuses several ranks while a
force of a single-rank family lives, whenever that force was created.

Two contexts of 8 atoms: one with a 3 nm box (every family but generalized Born), one without (generalized Born needs free space)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import cmap_cases as C  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import tables as T  # noqa: E402

N = 8
BOX = np.full(3, 3.0)
POS, TERMS = C.backbone(N, seed=7)
Q = np.array([0.3, -0.3] * (N // 2))
ZERO = np.zeros(N)
MAP = C.random_map(5, 21)
COEFFS = T.cmap_coefficients(*MAP).reshape(-1)
BONDS = np.stack([np.arange(N - 1), np.arange(1, N)], axis=1)

# per family: noun phrase, entry-point prefix, the wording of its bad-id refusal, whether that wording comes behind "<entry point>: ",
# and its cheap id-taking entry points as (name, call(ctx, id)) -- the last one the release where the family has one
FAMILIES = {
    'PAIR': ('a pair force', 'amm_pair_*', 'invalid pair force id', False,
             [('amm_pair_set_params', lambda c, i: c.pair_set_params(i, ZERO, ZERO, ZERO))]),
    'BONDED': ('a bond-list set', 'amm_bonded_*', 'invalid bonded force id', False,
               [('amm_bonded_finalize', lambda c, i: c.bonded_finalize(i)), ('amm_bonded_release', lambda c, i: c.bonded_release(i))]),
    'PME': ('a PME force', 'amm_pme_*', 'not a PME force id', False,
            [('amm_pme_set_charges', lambda c, i: c.pme_set_charges(i, ZERO))]),
    'TERM_EXPR': ('a term-expression force', 'amm_term_expr_*', 'not a term-expression force id', True,
                  [('amm_term_expr_set_globals', lambda c, i: c.term_expr_set_globals(i, [])),
                   ('amm_term_expr_release', lambda c, i: c.term_expr_release(i))]),
    'CV': ('a collective-variable force', 'amm_cv_*', 'not the id of a collective-variable force (AMM_FORCE_CV)', True,
           [('amm_cv_set_globals', lambda c, i: c.cv_set_globals(i, [])), ('amm_cv_release', lambda c, i: c.cv_release(i))]),
    'COMPOUND': ('a compound-bond force', 'amm_compound_*', 'not the id of a compound-bond force (AMM_FORCE_COMPOUND)', True,
                 [('amm_compound_set_globals', lambda c, i: c.compound_set_globals(i, [])),
                  ('amm_compound_release', lambda c, i: c.compound_release(i))]),
    'GB': ('a generalized-Born force', 'amm_gb_*', 'not the id of a generalized-Born force (AMM_FORCE_GB)', True,
           [('amm_gb_set_params', lambda c, i: c.gb_set_params(i, Q, np.full(N, 0.15), np.full(N, 0.8))),
            ('amm_gb_release', lambda c, i: c.gb_release(i))]),
    'CMAP': ('a CMAP force', 'amm_cmap_*', 'not the id of a CMAP force (AMM_FORCE_CMAP)', True,
             [('amm_cmap_set_params', lambda c, i: c.cmap_set_params(i, COEFFS, [0] * len(TERMS), 1)),
              ('amm_cmap_release', lambda c, i: c.cmap_release(i))]),
}
RELEASABLE = [name for name, spec in FAMILIES.items() if spec[4][-1][0].endswith('_release')]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def evaluate(ctx, fid, pos=POS):
    f = dev(np.zeros((N, 3)))
    e = torch.zeros(1, dtype=torch.float64, device='cuda')
    ctx.force_eval(fid, dev(pos), f, accumulate=False, energy=e)
    ctx.synchronize()
    return e.item(), f.cpu().numpy()


def bond_list(ctx, k=800.0):
    fid = ctx.bonded_create()
    ctx.bonded_add_terms(fid, B.BOND_HARMONIC, BONDS, np.stack([np.full(N - 1, 0.14), np.full(N - 1, k)], axis=1))
    ctx.bonded_finalize(fid)
    return fid


def create(ctx, family):
    """One small object of `family` on `ctx`; every one of them has forces that are not zero at POS."""
    if family == 'PAIR':
        return ctx.pair_create(B.pair_desc(B.NEAR_NONE, 1.0, rc0=1.0, rs0=0.8), Q, np.full(N, 0.2), np.full(N, 0.1))
    if family == 'BONDED':
        return bond_list(ctx)
    if family == 'PME':
        return ctx.pme_create(3.0, [5, 5, 5], Q)                  # (five points per axis: the smallest mesh the library takes)
    if family == 'TERM_EXPR':
        prog = X.compile_term('1.5*x*x + y - 2*z', ('x', 'y', 'z'), [], [])
        rows = np.full((N, 4), -1, dtype=np.int32)
        rows[:, 0] = np.arange(N)
        return ctx.term_expr_create(B.TERM_EXTERNAL, prog.code, prog.consts, [], rows, np.zeros((0, 1)))
    if family == 'CV':
        prog = X.compile_cv('2*cv1', ['cv1'], [], [])
        return ctx.cv_create([bond_list(ctx, k=650.0)], 0, prog.code, prog.consts, [])
    if family == 'COMPOUND':
        prog = X.compile_compound('distance(p1,p2)', 2, 'p', [], [])[0]
        return ctx.compound_create(2, prog.code, prog.consts, [], [B.CVAR_DISTANCE], [[0, 1]], np.array([[0, 1]], dtype=np.int32), np.zeros((0, 1)))
    if family == 'GB':
        return ctx.gb_create(Q, np.full(N, 0.15), np.full(N, 0.8))
    assert family == 'CMAP'
    return ctx.cmap_create([MAP[0]], COEFFS, [0] * len(TERMS), TERMS[:, 1:])


def refusal(family, entry, owner=None, fid=None):
    """The message an entry point of `family` gives an id that is not its own: bare for a released or unknown id, naming the owner of
    a live one."""
    _, _, wording, names_itself, _ = FAMILIES[family]
    text = (entry + ': ' if names_itself else '') + wording
    if owner is not None:
        noun, prefix = FAMILIES[owner][:2]
        text += ': force %d is %s (AMM_FORCE_%s: %s)' % (fid, noun, owner, prefix)
    return text


def test_every_family_names_the_owner_of_a_foreign_id_and_changes_nothing():
    box, free = B.HipContext(N, BOX), B.HipContext(N, None)
    try:
        home = {name: (free if name == 'GB' else box) for name in FAMILIES}
        ids = {name: create(home[name], name) for name in FAMILIES}
        before = {name: evaluate(home[name], ids[name]) for name in FAMILIES}
        for name, (e, f) in before.items():
            assert np.isfinite(e) and np.isfinite(f).all() and np.abs(f).max() > 0.0, name
        n_calls = 0
        for owner in FAMILIES:
            for family, spec in FAMILIES.items():
                if family == owner:
                    continue
                for entry, call in spec[4]:
                    with pytest.raises(B.HipError) as err:
                        call(home[owner], ids[owner])
                    assert str(err.value) == refusal(family, entry, owner, ids[owner]), (owner, entry)
                    n_calls += 1
        assert n_calls == 7 * (8 + len(RELEASABLE))            # 56 ordered pairs, the releases on top
        for name in FAMILIES:
            e, f = evaluate(home[name], ids[name])
            assert e == before[name][0] and np.array_equal(f, before[name][1]), name
        # an id that no force has: the bare wording
        with pytest.raises(B.HipError) as err:
            box.cmap_release(len(FAMILIES) + 100)
        assert str(err.value) == refusal('CMAP', 'amm_cmap_release')
        box.check()
        free.check()
    finally:
        box.close()
        free.close()


def test_a_released_id_is_refused_and_leaves_its_groups():
    """Every family with a release lives without a box.  One group holds a bond-list set that stays and one force of each of them; they
    are released one by one."""
    ctx = B.HipContext(N, None)
    try:
        keep = bond_list(ctx, k=500.0)
        ids = {name: create(ctx, name) for name in RELEASABLE}
        single = {name: evaluate(ctx, fid)[1] for name, fid in ids.items()}
        f_keep = evaluate(ctx, keep)[1]
        x, v, m = dev(POS), dev(np.zeros((N, 3))), dev(np.ones(N))
        buf = dev(np.full((N, 3), np.nan))
        ctx.bind_state(x, v, m)
        ctx.bind_buffer(0, buf)
        ctx.group_define(0, 0, [keep] + [ids[name] for name in RELEASABLE])

        def group_forces():
            buf.fill_(float('nan'))
            ctx.run_ops([B.Op(B.OP_EVAL, 0, 0, 0, 0.0)], 1)          # (refused as a released id if the group still listed one)
            ctx.synchronize()
            return buf.cpu().numpy()

        def assert_sum_of(members):
            # the group's buffer is the sum of its members in the order given: 7 additions at the most, each within half an ulp of
            # the partial sum, and a member adds the numbers it writes when evaluated alone -- 8 ulp of the largest partial sum
            total, scale = f_keep.copy(), np.abs(f_keep)
            for name in members:
                total, scale = total + single[name], scale + np.abs(single[name])
            assert np.abs(group_forces() - total).max() <= 8 * 2.0 ** -52 * scale.max()

        alive = list(RELEASABLE)
        assert_sum_of(alive)
        for name in RELEASABLE:
            entry, release = FAMILIES[name][4][-1]
            release(ctx, ids[name])
            alive.remove(name)
            for own_entry, call in FAMILIES[name][4]:
                with pytest.raises(B.HipError) as err:
                    call(ctx, ids[name])
                assert str(err.value) == refusal(name, own_entry), own_entry
            with pytest.raises(B.HipError, match='released force id'):
                evaluate(ctx, ids[name])
            assert_sum_of(alive)
        ctx.check()
    finally:
        ctx.close()


def set_slice(ctx, rank, world):
    B._chk(B.lib().amm_set_slice(ctx.h, rank, world))


def test_set_slice_refuses_a_single_rank_family_created_before_it():
    ctx = B.HipContext(N, BOX)
    try:
        ids = {name: create(ctx, name) for name in ('PAIR', 'BONDED', 'PME', 'CV', 'COMPOUND', 'CMAP')}
        for name in ('CV', 'COMPOUND', 'CMAP'):                      # the first such force is named, in GB's wording
            with pytest.raises(B.HipError) as err:
                set_slice(ctx, 0, 2)
            assert str(err.value) == 'amm_set_slice: %s (AMM_FORCE_%s) runs on a single rank' % (FAMILIES[name][0], name)
            FAMILIES[name][4][-1][1](ctx, ids[name])                 # released: the next one's turn
        set_slice(ctx, 0, 2)                                         # what is left slices
        set_slice(ctx, 0, 1)
        ctx.check()
    finally:
        ctx.close()
    sliced = B.HipContext(N, BOX)
    try:
        for name in ('PAIR', 'BONDED', 'PME'):                       # a context that never held another family
            create(sliced, name)
        set_slice(sliced, 0, 2)
    finally:
        sliced.close()
    free = B.HipContext(N, None)
    try:
        create(free, 'GB')
        with pytest.raises(B.HipError, match=r'amm_set_slice: a generalized-Born force \(AMM_FORCE_GB\) runs on a single rank'):
            set_slice(free, 0, 2)
    finally:
        free.close()
