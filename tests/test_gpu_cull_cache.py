"""The cull pre-pass's cached tree (lens-flare_amd/csrc/lf_cull_prepass.hip: k_cull_level_build, k_cull_resolve; no
reference counterpart).  Everything the pre-pass decides before a box's last test is independent of the sun; a context keeps it --
per level a slot per (path, own block, cell) and the exit footprints of the undecided boxes -- and a launch with a new sun
resolves its table from that in one pass.  What must hold, and is held here:

  * the table and the started fraction are those of the pre-pass that marches its boxes at every build
    (lf_test_knob("cull_cache", 0)), bit for bit, whatever the sun and the level structure;
  * the tree is built once per static key (lens, frame, mask, pairs, share) and rebuilt exactly once when one of them changes;
  * a tree beyond the byte budget, a test's rules, and a host that changes the key at every launch fall back to the
    uncached pre-pass without building.

The table is read after a launch that marches one tile row only (set_band(0, 8)): the pre-pass does not depend on the band."""
import numpy as np
import pytest

from goldenlib import load_texels

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
MASK = "pentbig500_14.png"
# the default, a wide sun (boxes lose samples), a small lobe, a sun off the frame
SUNS = [([0.01533, 0.0069, -1.0], 0.05), ([-0.15, 0.2, -1.0], 0.2), ([0.05, 0.02, -1.0], 0.004), ([0.9, 0.35, -1.0], 0.05),
        ([-0.02, 0.03, -1.0], 0.05)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture()
def forced(pkg):
    """the culled march whatever the table starts, on every context created meanwhile (frames this small start more than
    the fraction above which a launch takes the path tree by itself)"""
    pkg.test_knob_default("cull_force", 1)
    yield
    pkg.test_knob_default("cull_force", 0)


@pytest.fixture()
def lf(pkg, forced):
    """a context of its own per test: the cache's policy remembers what a context was asked before"""
    ctx = pkg.LensFlare(0)
    ctx.set_cull_audit(0)
    ctx.timing_enable(True)
    yield ctx
    ctx.close()


def _lens(pkg, name="dgauss11.lens"):
    lens = pkg.load_lens_file(name)
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if "lambda_nm" in lens else None
    return lens, lam


def _setup(pkg, lf, W, H, lens_name="dgauss11.lens", lens=None, lam=None, mask=MASK, pairs=None, primary=True, sun=SUNS[0]):
    if lens is None:
        lens, lam = _lens(pkg, lens_name)
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, load_texels(mask))
    lf.set_lens(lens)
    if lam is not None:
        lf.set_lambda_rgb(lam)
    lf.set_sun(sun[0], RAD, sun[1])
    lf.set_ghost_pairs(pairs, primary)
    lf.set_row_interleave(0, 1)
    lf.set_band(0, 8)
    lf.set_march_culling(2)


def _table(lf, spp, cache, key=1):
    """the table of one launch (mode 2: a pre-pass per launch), the cached tree on or off"""
    lf.test_knob("cull_cache", 1 if cache else 0)
    try:
        lf.trace_ghosts(spp, key)
    finally:
        lf.test_knob("cull_cache", 1)
    assert lf.cull_info()["culled"] and lf.cull_reason() == "applied", lf.cull_reason()
    return lf.cull_table(), lf.cull_started_fraction()


def _builds(lf):
    lf.synchronize()
    return lf.timing_get("cull_cache_build")[0]


def _same(lf, spp, key=1):
    """cached and uncached table of the context's present inputs are equal -> the table"""
    tc, fc = _table(lf, spp, True, key)
    tu, fu = _table(lf, spp, False, key)
    assert np.array_equal(tc, tu) and fc == fu, (fc, fu, int((tc != tu).sum()))
    return tc, fc


# frame, samples, block side, P, levels (the level structures that can go wrong), lens
SHAPES = [(400, 224, 16, 16, 16, 2, "dgauss11.lens"),
          (640, 360, 64, 32, 32, 3, "dgauss11.lens"),
          (1280, 720, 256, 64, 64, 4, "dgauss11.lens"),          # the bench's structure at 240 blocks
          (640, 360, 36, 32, 24, 2, "dgauss11_8lambda.lens"),
          (640, 360, 1, 32, 4, 1, "dgauss11.lens")]


@pytest.mark.parametrize("W,H,spp,block,P,n_levels,lens_name", SHAPES)
def test_same_table_as_the_sun_moves(pkg, lf, W, H, spp, block, P, n_levels, lens_name):
    _setup(pkg, lf, W, H, lens_name)
    lf.timing_reset()
    fracs = []
    for sun, alpha in SUNS:
        lf.set_sun(sun, RAD, alpha)
        t, f = _same(lf, spp)
        info = lf.cull_info()
        assert info["block_px"] == block and info["P"] == P
        fracs.append((f, bool(t.any())))
    print(f"{W}x{H} {spp} spp {lens_name}: started fraction per sun {[round(f, 5) for f, _ in fracs]}")
    assert _builds(lf) == 1
    assert lf.timing_get("cull_prepass")[0] == 2 * len(SUNS)          # one per launch, cached or not
    assert fracs[0][1] and 0.0 < fracs[0][0] < 1.0 and len({f for f, _ in fracs}) > 1     # it culls, and the sun matters
    levels = [P]
    while levels[0] % 2 == 0 and levels[0] // 2 >= 8:
        levels.insert(0, levels[0] // 2)
    assert len(levels) == n_levels


def test_same_frame(pkg, lf):
    W, H, spp = 400, 224, 16
    _setup(pkg, lf, W, H)
    lf.set_band(0, H)
    got = {}
    for cache in (1, 0, 1):
        lf.test_knob("cull_cache", cache)
        lf.reset_counters()
        lf.trace_ghosts(spp, 11)
        assert lf.cull_info()["culled"]
        now = (lf.read_buffer(pkg.GHOST_BUFFER), lf.counters(), lf.march_stats())
        if cache in got:
            assert np.array_equal(now[0], got[cache][0])
        got[cache] = now
    assert got[1][0].max() > 0 and np.array_equal(got[1][0], got[0][0])
    assert got[1][1] == got[0][1] and got[1][2] == got[0][2]
    assert _builds(lf) == 1


def test_every_static_input_invalidates_once(pkg, lf):
    spp = 64
    lens, _ = _lens(pkg)
    state = dict(W=640, H=360, lens=lens, lam=None, mask=MASK, pairs=None, primary=True)

    def apply(**kw):
        state.update(kw)
        _setup(pkg, lf, **state)

    apply()
    first, _ = _same(lf, spp)
    assert _builds(lf) == 1
    seen = [first]

    def changed(what, expect_other_table=True):
        n0 = _builds(lf)
        t, _ = _same(lf, spp)            # builds, then the uncached table
        _table(lf, spp, True)            # ... and reuses
        assert _builds(lf) == n0 + 1, what
        if expect_other_table:
            assert all(t.shape != s.shape or not np.array_equal(t, s) for s in seen[-1:]), what
        seen.append(t)

    apply(mask="octagonbokeh.png"); changed("another mask")
    refocused = dict(lens)
    refocused["thickness"] = lens["thickness"].copy()
    refocused["thickness"][-1] += 1.5
    apply(lens=refocused); changed("a refocused lens")
    lens8, lam8 = _lens(pkg, "dgauss11_8lambda.lens")
    apply(lens=lens8, lam=lam8); changed("another lens file")
    apply(lens=lens, lam=None); changed("the first lens again")
    apply(W=400, H=224); changed("another frame size")
    apply(pairs=[(1, 3), (0, 2), (6, 8), (2, 9)], primary=False); changed("a pair subset")
    apply(pairs=None, primary=True); changed("all pairs again")
    lf.set_mask_filter(pkg.MASK_BILINEAR); changed("lf_set_mask_filter", expect_other_table=False)
    lf.set_mask_filter(pkg.MASK_NEAREST)


def test_block_deal_invalidates_and_ranks_build_their_own_rows(pkg, lf):
    """two contexts as ranks 0 and 1 of a block deal on one device: each rank's own rows are the uncached ones -- and those
    of the whole table a single context builds"""
    W, H, spp = 1280, 720, 256
    _setup(pkg, lf, W, H)
    whole, _ = _same(lf, spp)
    assert _builds(lf) == 1
    by, bx = whole.shape[:2]
    other = pkg.LensFlare(0)
    try:
        other.set_cull_audit(0)
        other.timing_enable(True)
        _setup(pkg, other, W, H)
        for rank, ctx in ((1, lf), (0, other)):
            ctx.set_block_deal(rank, 2)
            n0 = _builds(ctx)
            t, _ = _same(ctx, spp)
            _table(ctx, spp, True)
            assert _builds(ctx) == n0 + 1
            flat, ref = t.reshape(by * bx, -1), whole.reshape(by * bx, -1)
            own = np.arange(by * bx) % 2 == rank
            assert np.array_equal(flat[own], ref[own]) and ref[own].any()
    finally:
        other.close()


def test_fallbacks(pkg, lf):
    W, H, spp = 400, 224, 16
    _setup(pkg, lf, W, H)
    ref, fref = _table(lf, spp, False)
    # a tree beyond the budget: today's path
    lf.test_knob("cull_cache_max_mb", 1)
    for _ in range(2):
        t, f = _table(lf, spp, True)
        assert np.array_equal(t, ref) and f == fref and lf.cull_reason() == "applied"
    assert _builds(lf) == 0
    lf.test_knob("cull_cache_max_mb", 8192)
    # a rule knob: the general kernel, nothing cached
    lf.test_knob("cull_lobe_k", 1.2)
    try:
        t, f = _table(lf, spp, True)
        assert np.array_equal(t, ref) and f == fref
        assert _builds(lf) == 0
    finally:
        lf.test_knob("cull_general_kernel", 0)
    t, f = _table(lf, spp, True)
    assert np.array_equal(t, ref) and f == fref and _builds(lf) == 1


def test_a_budget_for_the_slots_but_not_the_footprints(pkg, lf):
    """a build that has STARTED gives up: the budget admits the slots of every level and some 200 footprints, the first level
    appends about 1e6 (the kernel counts them all and writes those below its capacity).  The launch takes the uncached
    pre-pass; the key is remembered as one that does not fit under this budget, and built under a larger one."""
    W, H, spp = 400, 224, 16
    lens, _ = _lens(pkg)
    _setup(pkg, lf, W, H)
    ref, fref = _table(lf, spp, False)
    info = lf.cull_info()
    glass = lens["n"] - 1                                    # all pairs of the interfaces that are not the stop, + the primary path
    paths = 1 + glass * (glass - 1) // 2
    levels = [info["P"]]
    while levels[0] % 2 == 0 and levels[0] // 2 >= 8:
        levels.insert(0, levels[0] // 2)
    assert len(levels) == 2 and info["block_px"] == 16
    slots_mb = 4.0 * paths * info["blocks_x"] * info["blocks_y"] * sum(P * P for P in levels) / 2.0 ** 20
    lf.test_knob("cull_cache_max_mb", slots_mb + 0.01)
    t, f = _table(lf, spp, True)
    n1 = _builds(lf)
    print(f"slots {slots_mb:.3f} MiB, {paths} paths, levels {levels}: cull_cache_build events after the first launch {n1}")
    assert np.array_equal(t, ref) and f == fref
    assert n1 == 1                                           # the build that began and gave up is timed
    t, f = _table(lf, spp, True)                             # the same key and budget: no second attempt
    assert np.array_equal(t, ref) and f == fref and _builds(lf) == n1
    lf.test_knob("cull_cache_max_mb", 8192)
    for _ in range(2):                                       # built once, then reused
        t, f = _table(lf, spp, True)
        assert np.array_equal(t, ref) and f == fref and _builds(lf) == n1 + 1


def test_a_key_that_changes_at_every_launch_is_not_rebuilt(pkg, lf):
    """a host that animates focus: four launches with four lenses build at most twice; a lens seen twice running is built"""
    W, H, spp = 400, 224, 16
    lens, _ = _lens(pkg)
    _setup(pkg, lf, W, H)
    last = None
    for k in range(4):
        moved = dict(lens)
        moved["thickness"] = lens["thickness"].copy()
        moved["thickness"][-1] += 0.25 * k
        lf.set_lens(moved)
        last, f = _table(lf, spp, True)
    n0 = _builds(lf)
    assert 1 <= n0 <= 2
    again, f2 = _table(lf, spp, True)          # the fourth lens a second time
    assert _builds(lf) == n0 + 1
    assert np.array_equal(again, last) and f2 == f
    unc, fu = _table(lf, spp, False)
    assert np.array_equal(again, unc) and f2 == fu
    n1 = _builds(lf)
    _table(lf, spp, True)                      # ... and reused from then on
    assert _builds(lf) == n1
