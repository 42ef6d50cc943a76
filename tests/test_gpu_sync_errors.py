"""gpe_sync waits once per stream and reads the sticky device-side error words through pinned words whose copies are
enqueued behind the context's work (check_device_errors): every synchronising entry point still reports the status and
the text it reported before, an error raised by the last enqueued step is seen by the gpe_sync that follows it, another
context of the process is not touched, and the pinned block is allocated once per context."""
import numpy as np
import pytest

DT = 1.0 / 60.0
LEFT_THE_BOX = "native collide: a particle left the world box between steps"


def _narrow_world(gpe):
    """The scene of test_gpu_cell_math.test_world_narrower_than_its_particles_matches_oracle: a world narrower than its
    largest particle, so the first NATIVE step's clamp puts every particle at x = W - r < 0, outside the cell box, and
    the second raises the sticky error on the device -- a flag word, nothing faults."""
    L = gpe._lib
    rng = np.random.default_rng(5)
    n = 41
    pos = np.stack([rng.uniform(0, 1, n), rng.uniform(0, 6, n)], 1).astype(np.float32)
    rad = rng.uniform(1.2, 3.0, n).astype(np.float32)
    rad[0] = 3.0
    st = gpe.State(pos, rad, world=(1.0, 6.0), gravity=(2.5, -9.81), mode=gpe.MODE_NATIVE, flags=L.FLAG_NATIVE_FORCE)
    info = st.ctx.pipeline_info()
    assert (info["pipeline"], info["reason"]) == (L.PIPELINE_NATIVE, L.REASON_NONE), info
    return st


def _cloud(gpe, n=4096, flags=0):
    world = (400.0, 300.0)
    pos, rad = gpe.scenes.uniform_cloud(n, world, seed=11)
    return gpe.State(pos, rad, world=world, mode=gpe.MODE_NATIVE, flags=flags)


@pytest.mark.gpu
def test_sticky_error_reaches_sync_and_downloads_and_no_other_context(gpe):
    L = gpe._lib
    other = _cloud(gpe)
    other.run(DT, 3, resort_every=0, resort_first=True)
    other.ctx.sync()
    st = _narrow_world(gpe)
    st.run(DT, 1, resort_every=0, resort_first=True)
    st.ctx.sync()                                               # the first step is clean
    assert (st.positions()[:, 0] < 0).all()
    st.update(DT)                                               # the last enqueued step raises the word ...
    with pytest.raises(L.GpeError) as err:
        st.ctx.sync()                                           # ... and the gpe_sync behind it sees it
    assert err.value.status == L.GPE_ERR_STATE and str(err.value) == "gpe status %d: %s" % (L.GPE_ERR_STATE, LEFT_THE_BOX)
    for read in (st.positions, st.previous_positions, st.ctx.sync):     # sticky: every synchronising entry point
        with pytest.raises(L.GpeError) as err:
            read()
        assert err.value.status == L.GPE_ERR_STATE and LEFT_THE_BOX in str(err.value), read
    assert L.load().gpe_last_error(st.ctx.h).decode() == LEFT_THE_BOX
    # the other context of the process: steps, synchronises and downloads as if nothing had happened
    plain = _cloud(gpe)
    plain.run(DT, 3, resort_every=0, resort_first=True)
    other.run(DT, 2, resort_every=0, resort_first=False)
    plain.run(DT, 2, resort_every=0, resort_first=False)
    other.ctx.sync()
    assert L.load().gpe_last_error(other.ctx.h).decode() == ""
    assert np.array_equal(other.positions(), plain.positions())
    assert np.array_equal(other.previous_positions(), plain.previous_positions())
    for s in (st, other, plain):
        s.close()


@pytest.mark.gpu
def test_the_pinned_error_words_are_allocated_once(gpe):
    """300 frames of gpe_step + gpe_sync: one "ctl.error_words" block in the registry from the first gpe_sync to the
    last, none released, and no device allocation made along the way."""
    st = _cloud(gpe)
    st.update(DT, resort=True)

    def blocks():
        return [(t, p, s, when) for t, p, s, when in st.ctx.guard_registry() if t == "ctl.error_words"]
    assert blocks() == []                                       # nothing has synchronised yet
    st.ctx.sync()
    assert blocks() == [("ctl.error_words", 64, 0, "pinned")]
    st.update(DT)
    st.ctx.sync()
    before = sorted(st.ctx.guard_registry())
    for _ in range(300):
        st.update(DT)
        st.ctx.sync()
    assert blocks() == [("ctl.error_words", 64, 0, "pinned")]
    assert sorted(st.ctx.guard_registry()) == before
    assert np.isfinite(st.positions()).all()
    st.close()
