"""Host-side logic of the engine that needs no GPU: channel chunking, sort size classes, the bounded size-guess cache."""
import pytest
import torch

from deblur4dgs_amd import engine


def test_channel_chunks_cover_every_count_with_instantiated_widths():
    for D in range(0, 70):
        ch = engine.channel_chunks(D)
        assert ch[0][0] == 0 and ch[-1][1] == D
        for (a, b, w), nxt in zip(ch, ch[1:] + [None]):
            assert w in engine.SUPPORTED_D and b - a <= w and (b - a == 16 or nxt is None)
            if nxt is not None:
                assert nxt[0] == b
        if D in engine.SUPPORTED_D:
            assert ch == [(0, D, D)]  # the common case: one pass, nothing padded
    # the reference's layouts: 3 + mask + 3B track channels (+ depth rides on the last chunk)
    assert engine.channel_chunks(16) == [(0, 16, 16)]
    assert engine.channel_chunks(3 + 1 + 18) == [(0, 16, 16), (16, 22, 8)]


def test_sort_classes_leave_headroom_and_fall_back_to_unknown():
    assert engine._sort_class(0) == 512 and engine._sort_class(341) == 512  # one wave, registers only (k_tile_sort_w)
    assert engine._sort_class(342) == 2048 and engine._sort_class(1365) == 2048
    assert engine._sort_class(1366) == 4096 and engine._sort_class(5000) == 8192 and engine._sort_class(10922) == 16384
    assert engine._sort_class(10923) == 0  # longer than the largest LDS class with 50 % headroom: every class is launched


def test_size_guess_cache_is_bounded_and_buckets_n():
    dev = torch.device("cuda", 0)  # only .index is used
    k1, k2 = engine._size_key(dev, 8, 300_000, 512, 288), engine._size_key(dev, 8, 310_000, 512, 288)
    assert k1 == k2  # densification moves N a little: same entry (two leading bits)
    assert engine._size_key(dev, 8, 600_000, 512, 288) != k1
    engine._SIZE_GUESS.clear()
    for i in range(3 * engine._SIZE_GUESS_MAX):
        engine._guess_put(("k", i), (i, 2048))
    assert len(engine._SIZE_GUESS) == engine._SIZE_GUESS_MAX
    assert engine._guess_get(("k", 0)) is None and engine._guess_get(("k", 3 * engine._SIZE_GUESS_MAX - 1)) is not None
    engine._SIZE_GUESS.clear()


def test_control_stats_sink_is_validated():
    import pytest

    good = {"xys_grad_norm_acc": torch.zeros(5), "vis_count": torch.zeros(5, dtype=torch.int64), "max_radii": torch.zeros(5),
            "batch_size": 2}
    assert engine._check_stats(good, 5) is good
    with pytest.raises(ValueError):
        engine._check_stats(good, 6)
    with pytest.raises(ValueError):
        engine._check_stats({**good, "vis_count": torch.zeros(5)}, 5)
    with pytest.raises(ValueError):
        engine._check_stats({**good, "batch_size": 0}, 5)


def test_deferred_records_queue_up_and_are_all_verified(monkeypatch):
    """Host logic of `deferred_size_check` without a GPU: several pending records per shape, every one is read, an
    overflow in ANY of them raises (only the newest used to survive)."""
    from deblur4dgs_amd import engine

    class Ev:
        def __init__(self, done):
            self.done = done

        def query(self):
            return self.done

        def synchronize(self):
            self.done = True

    # the records below carry ordinary host tensors: once read they would be recycled into the pool of PINNED count buffers that
    # later renders in this process draw from, so they go to a throwaway pool
    monkeypatch.setattr(engine, "_PINNED_FREE", [])
    key = ("unit", 1, 2, 3, 4)
    mk = lambda n, mt, live=0: torch.tensor([n, mt, 50, live], dtype=torch.int64)  # D4gsProjOut.n_isect: 50 sampled entries
    engine._DEFERRED[key] = [(mk(100, 10, 45), Ev(True), 200, 2048), (mk(900, 10, 50), Ev(True), 200, 2048),
                             (mk(120, 10, 10), Ev(False), 200, 2048)]
    with pytest.raises(RuntimeError, match="needed 900 intersections"):
        engine._deferred_poll(key)           # reads the two that have landed; the second one overflowed
    assert len(engine._DEFERRED[key]) == 1   # the pending one is still queued
    assert engine._guess_get(key)[0] >= 900  # the guess follows the largest count seen
    assert engine._LIVE_FRAC[key] == 45 / 50  # live fraction of the render that fitted (the overflowed one composited nothing)
    assert engine._deferred_poll(key) is None and len(engine._DEFERRED[key]) == 1  # not landed yet, non-blocking
    engine.check_deferred()                  # blocking drain: fits, no error
    assert key not in engine._DEFERRED
    assert engine._LIVE_FRAC[key] == 10 / 50
    engine._SIZE_GUESS.pop(key, None)
    engine._LIVE_FRAC.pop(key, None)


def test_row_mode_follows_the_measured_live_fraction(monkeypatch):
    """auto: the library's capacity heuristic until a render of that shape has been measured, then sparse below 50 % live."""
    from deblur4dgs_amd import _lib as L, engine

    dev = torch.device("cuda", 0)
    cfg = engine.RenderCfg(N=1000, G=0, K=0, T=0, S=2, D=3, width=64, height=48)
    key = engine._size_key(dev, 2, 1000, 64, 48)
    engine._LIVE_FRAC.pop(key, None)
    assert engine.row_mode_for(cfg, dev) == L.ROWS_AUTO
    engine._live_put(key, 150, 1000)
    assert engine.row_mode_for(cfg, dev) == L.ROWS_SPARSE
    engine._live_put(key, 930, 1000)
    assert engine.row_mode_for(cfg, dev) == L.ROWS_DENSE
    monkeypatch.setattr(engine, "BWD_ROWS", "sparse")
    assert engine.row_mode_for(cfg, dev) == L.ROWS_SPARSE
    engine._LIVE_FRAC.pop(key, None)


def test_exact_tiles_auto_keeps_one_size_guess_per_flag_and_counts_again_after_on_to_off(monkeypatch):
    """with D4GS_EXACT_TILES=auto the lists binned under the flag are 15-40 % shorter; the capacity measured with the
    flag on must never size a render that runs with it off.  The guesses are keyed on the resolved flag, an on -> off flip
    leaves NO guess for the off key (the next render counts first, also under deferred_size_check), and the live-fraction
    condition has hysteresis."""
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(engine, "EXACT_TILES", "auto")
    monkeypatch.setattr(engine, "seg_state_elems", lambda cfg: 0)
    S, N, W, H = 2, 1000, 640, 480
    base = engine._size_key(dev, S, N, W, H)
    mk = lambda: engine.RenderCfg(N=N, G=0, K=0, T=0, S=S, D=3, width=W, height=H)
    cap = lambda per_inst: int(per_inst * S * N * 1.25) + 4096
    for k in (base + (False,), base + (True,)):
        engine._guess_drop(k)
    engine._XT_ON.pop(base, None)
    engine._LIVE_FRAC.pop(base, None)
    try:
        cfg = engine.resolve_lazy(mk(), dev)
        assert cfg.exact_tiles is False and engine._list_key(dev, cfg) == base + (False,)  # nothing measured yet
        engine._guess_put(base + (False,), (cap(4.0), 2048))  # rectangles: 4 intersections per instance -> on
        cfg = engine.resolve_lazy(mk(), dev)
        assert cfg.exact_tiles is True and engine._list_key(dev, cfg) == base + (True,)
        assert engine._guess_get(engine._list_key(dev, cfg)) is None  # the render with the flag on does not inherit the off capacity
        engine._guess_put(base + (True,), (cap(2.8), 512))  # what that render measured: shorter lists, a smaller sort class
        engine._live_put(base, 45, 100)                      # 45 % live: below the 0.5 that turns it on, above the 0.4 that turns it off
        assert engine.resolve_lazy(mk(), dev).exact_tiles is True
        engine._live_put(base, 30, 100)                      # now it goes off ...
        cfg = engine.resolve_lazy(mk(), dev)
        assert cfg.exact_tiles is False
        assert engine._guess_get(engine._list_key(dev, cfg)) is None  # ... and the stale off-key capacity is gone: count first
        assert engine._guess_get(base + (True,)) == (cap(2.8), 512)    # a late deferred record of the on-render lands under ITS key
        engine._live_put(base, 45, 100)
        engine._guess_put(base + (False,), (cap(4.0), 2048))
        assert engine.resolve_lazy(mk(), dev).exact_tiles is False     # 45 % does not turn it back on
    finally:
        for k in (base + (False,), base + (True,)):
            engine._guess_drop(k)
        engine._XT_ON.pop(base, None)
        engine._LIVE_FRAC.pop(base, None)


# ---- the list-size protocol, rule by rule.  Expected capacities and sort classes come from tests/ladder.py (its own statements of
# the rules), count buffers are ordinary host int64[4] tensors and go back to a throwaway pool, no GPU is touched.

class _Ev:
    """What the protocol uses of a torch.cuda.Event (as in test_deferred_records_queue_up_and_are_all_verified)."""

    def __init__(self, done=True):
        self.done = done

    def query(self):
        return self.done

    def synchronize(self):
        self.done = True


def _counts(n, max_tile, live=0, sampled=50):
    return torch.tensor([n, max_tile, sampled, live], dtype=torch.int64)  # D4gsProjOut.n_isect


@pytest.fixture
def size_state(monkeypatch):
    """A throwaway pinned pool; the keys a test registers here leave no guess, live fraction or record behind."""
    monkeypatch.setattr(engine, "_PINNED_FREE", [])
    keys = []
    yield keys
    for k in keys:
        engine._guess_drop(k)
        engine._LIVE_FRAC.pop(k[:5], None)
        engine._DEFERRED.pop(k, None)
        engine._XT_ON.pop(k[:5], None)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4095, 4096, 4097, 10**6 + 3])
def test_stored_capacity_is_the_ladders_warm_capacity(n, size_state):
    from tests import ladder

    key = ("cap", 0, n, 3, 4, False)
    size_state.append(key)
    engine._DEFERRED[key] = [(_counts(n, 10), _Ev(), n, 0)]
    assert engine._deferred_poll(key) == (n, 10)
    assert engine._guess_get(key) == (ladder.warm_capacity(n), ladder.sort_class(10))


def test_deferred_poll_overflowed_record_is_not_the_newest(size_state):
    from tests import ladder

    key = ("unit", 2, 2, 3, 4, False)
    size_state.append(key)
    b1, b2 = _counts(900, 3000, live=50), _counts(100, 10, live=20)
    engine._DEFERRED[key] = [(b1, _Ev(), 200, 2048), (b2, _Ev(), 200, 2048)]
    with pytest.raises(RuntimeError, match="needed 900 intersections"):
        engine._deferred_poll(key)
    assert key not in engine._DEFERRED
    # the newest record sets the guess, the overflowed one raises it: its capacity, the class of the longer of the two longest lists
    assert engine._guess_get(key) == (ladder.warm_capacity(900), ladder.sort_class(3000))
    assert engine._LIVE_FRAC[key[:5]] == 20 / 50  # the second record's only: the overflowed render composited nothing
    assert len(engine._PINNED_FREE) == 2 and engine._PINNED_FREE[0] is b1 and engine._PINNED_FREE[1] is b2


def test_deferred_poll_longest_list_overflow_alone(size_state):
    from tests import ladder

    key = ("unit", 3, 2, 3, 4, False)
    size_state.append(key)
    engine._DEFERRED[key] = [(_counts(100, 3000, live=40), _Ev(), 200, 2048)]
    with pytest.raises(RuntimeError, match=r"needed 100 intersections \(longest tile list 3000\).*sized for 200 \(class 2048\)"):
        engine._deferred_poll(key)
    assert key[:5] not in engine._LIVE_FRAC
    assert engine._guess_get(key) == (ladder.warm_capacity(100), ladder.sort_class(3000))
    engine._DEFERRED[key] = [(_counts(100, 3000, live=40), _Ev(), 200, 0)]  # hint 0 = class unknown: every class was launched
    assert engine._deferred_poll(key) == (100, 3000)
    assert engine._LIVE_FRAC[key[:5]] == 40 / 50


def test_graph_watch_check_updates_overflowed_guesses_only(size_state):
    from tests import ladder

    fits, by_count, by_list = (("unit", 4, i, 3, 4, False) for i in range(3))
    size_state.extend((fits, by_count, by_list))
    for k in (fits, by_count, by_list):
        engine._guess_put(k, (1234, 2048))
    watch = object.__new__(engine.GraphWatch)  # (__init__ pins memory)
    watch.recs = [(fits, _counts(150, 100, live=30), 200, 2048), (by_count, _counts(700, 100, live=50), 200, 2048),
                  (by_list, _counts(120, 2500, live=50), 200, 2048)]
    watch.event = _Ev(False)
    with pytest.raises(RuntimeError, match=r"needed 700 intersections \(longest tile list 100\).*captured with lists for 200 \(class 2048\)"):
        watch.check()
    assert engine._guess_get(fits) == (1234, 2048)
    assert engine._guess_get(by_count) == (ladder.warm_capacity(700), ladder.sort_class(100))
    assert engine._guess_get(by_list) == (ladder.warm_capacity(120), ladder.sort_class(2500))
    assert engine._LIVE_FRAC[fits[:5]] == 30 / 50
    assert by_count[:5] not in engine._LIVE_FRAC and by_list[:5] not in engine._LIVE_FRAC
    assert watch.event is None
    watch.check()  # nothing replayed since: a no-op


def test_lazy_sort_auto_decides_from_the_capacity_with_its_constant_left_in(monkeypatch, size_state):
    """LAZY_AUTO_KEYS and the near_target factor were tuned on `capacity / 1.25` per tile list - the 4096 of the capacity rule is
    NOT taken out first.  The guesses sit so close to the line that taking it out would flip the decision."""
    import math

    dev = torch.device("cuda", 0)
    monkeypatch.setattr(engine, "LAZY_SORT", "auto")
    monkeypatch.setattr(engine, "EXACT_TILES", "0")
    S, N, W, H = 2, 1000, 64, 48
    mk = lambda: engine.RenderCfg(N=N, G=0, K=0, T=0, S=S, D=3, width=W, height=H)
    tw, th = mk().tiles
    lists = S * tw * th
    base = engine._size_key(dev, S, N, W, H)
    size_state.append(base + (False,))
    size_state.append(base + (True,))
    on_from = math.ceil(engine.LAZY_AUTO_KEYS * 1.25 * lists)
    assert on_from / 1.25 / lists >= engine.LAZY_AUTO_KEYS > (on_from - 1) / 1.25 / lists
    assert (on_from + 4000 - 4096) / 1.25 / lists < engine.LAZY_AUTO_KEYS  # without the constant both "on" guesses would be off
    low, high = engine.LAZY_AUTO_LIVE / 2, (1 + engine.LAZY_AUTO_LIVE) / 2
    for cap, f, want in ((on_from, low, True), (on_from + 4000, low, True), (on_from - 1, low, False), (on_from, high, False),
                         (10 * on_from + 7, 0.3 * engine.LAZY_AUTO_LIVE, True)):
        engine._guess_put(base + (False,), (cap, 2048))
        engine._live_put(base, int(f * 10000), 10000)
        f = engine._LIVE_FRAC[base]
        cfg = engine.resolve_lazy(mk(), dev)
        assert cfg.exact_tiles is False
        assert (f < engine.LAZY_AUTO_LIVE and cap / 1.25 / lists >= engine.LAZY_AUTO_KEYS) == want, (cap, f)  # (the cases are what they claim)
        assert cfg.lazy_sort is want, (cap, f)
        assert cfg.near_target == (max(256, int(2.5 * f * cap / 1.25 / lists)) if want else 0), (cap, f)
    engine._guess_drop(base + (False,))  # nothing measured: off, whatever the live fraction
    assert engine.resolve_lazy(mk(), dev).lazy_sort is False


def test_frame_supported_caps_the_sub_samples_of_a_blended_frame():
    """The one-call path's winner map is one signed byte per pixel and channel: candidates 0 .. S - 2 <= 127, i.e. S <= 129 with a
    blended frame (include/d4gs.h, D4GS_FRAME_BLEND_MAX_S); an unblended frame has no map and no cap."""
    import os
    import re

    mk = lambda S, D=3, N=100: engine.RenderCfg(N=N, G=0, K=0, T=0, S=S, D=D, width=16, height=16)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d4gs.h")).read()
    assert int(re.search(r"#define\s+D4GS_FRAME_BLEND_MAX_S\s+(\d+)", hdr).group(1)) == engine.FRAME_BLEND_MAX_S == 129
    assert engine.FRAME_BLEND_MAX_S - 2 == 127  # the last candidate's index is the largest int8_t
    for S in (1, 11, 128, 129):
        assert engine.frame_supported(mk(S)) and engine.frame_supported(mk(S), blended=True) and engine.frame_supported(mk(S), blended=False)
    for S in (130, 131, 257, 1000):
        assert not engine.frame_supported(mk(S)) and not engine.frame_supported(mk(S), blended=True)
        assert engine.frame_supported(mk(S), blended=False)
    assert not engine.frame_supported(mk(3, N=0)) and not engine.frame_supported(mk(3, D=22), blended=False)  # (as before)


def test_one_call_entry_points_refuse_a_blended_frame_of_more_than_129_sub_samples():
    """d4gs_forward / d4gs_backward return D4GS_EINVAL with a message before any HIP call (the fake addresses are never dereferenced)."""
    import ctypes as C

    from deblur4dgs_amd import _lib as L
    from tests.test_absgrad_abi import FAKE, _frame_args

    lib = L.lib()
    d, pin, io, leaf = _frame_args(0)
    io.blended, io.acc = FAKE, FAKE
    fg = L.FrameGrads(v_blended=FAKE, v_means2d=FAKE)
    ws = C.c_void_p(FAKE)
    for S, refused in ((129, False), (130, True)):
        d.S = S
        rc = lib.d4gs_forward(C.byref(d), C.byref(pin), C.byref(io), ws, 0, 1000, 0, None)
        rcb = lib.d4gs_backward(C.byref(d), C.byref(pin), C.byref(io), C.byref(fg), C.byref(leaf), ws, 0, 1000, 0, None)
        msg = lib.d4gs_last_error()
        if refused:
            assert rc == -1 and rcb == -1 and b"at most 129" in msg, (rc, rcb, msg)
        else:  # passes the cap and stops at the next check: the workspace of 0 bytes
            assert rc != 0 and rcb != 0 and b"workspace" in msg, (rc, rcb, msg)
    d.S = 130
    io.blended, io.acc = None, None  # no blend, no map, no cap
    assert lib.d4gs_forward(C.byref(d), C.byref(pin), C.byref(io), ws, 0, 1000, 0, None) != 0
    assert b"workspace" in lib.d4gs_last_error(), lib.d4gs_last_error()
