"""Self-tests of tests/guardband.py on CPU tensors: a Python function stands in for the C-ABI entry point.  Each test fails
when the check of guardband.py it is about is taken out (band comparison, grouping, alignment, copy-back, replay)."""
import pytest
import torch

import guardband as G


def guarded(replay=False):
    return G.GuardedCalls(replay=replay, install=False)


def test_clean_stand_in_passes_and_the_originals_hold_its_results():
    x = torch.arange(10, dtype=torch.float32)
    out = torch.zeros(10)
    tbl = torch.zeros(4, dtype=torch.int32)
    d = torch.zeros(3, dtype=torch.float64)
    seen = {}

    def entry(args):
        a, o, t, dd, none, n = args
        assert none is None and n == 10
        seen['ptrs'] = (a.data_ptr(), o.data_ptr())
        o.copy_(a * 2)
        t.copy_(torch.tensor([1, 2, 3, 4], dtype=torch.int32))
        dd.fill_(0.1)

    with guarded(replay=True) as g:
        g.run('stand_in', 'pppppi', (x, out, tbl, d, None, 10), entry)
    assert g.calls == 1 and 'stand_in' in G.GUARDED_NAMES
    assert seen['ptrs'][0] != x.data_ptr() and seen['ptrs'][1] != out.data_ptr()      # it ran on relocated tensors
    assert torch.equal(out, x * 2) and tbl.tolist() == [1, 2, 3, 4] and torch.equal(d, torch.full((3,), 0.1, dtype=torch.float64))
    assert torch.equal(x, torch.arange(10, dtype=torch.float32))


def _raw_words(t, lo, hi):
    """int32 view of the words [lo, hi) around the start of the relocated tensor t, inside its guarded allocation."""
    st = t.untyped_storage()
    whole = torch.empty(0, dtype=torch.int32).set_(st, 0, (st.nbytes() // 4,))
    at = t.storage_offset() * t.element_size() // 4
    return whole[at + lo:at + hi]


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32])
@pytest.mark.parametrize('where', ['behind', 'in front of'])
def test_one_word_outside_the_output_is_caught_and_attributed(where, dtype):
    x = torch.ones(7)
    out = torch.zeros(33, dtype=dtype)

    def entry(args):
        a, o, n = args
        o.fill_(5)
        if where == 'behind':
            _raw_words(o, 33, 34).fill_(123)
        else:
            _raw_words(o, -1, 0).fill_(123)

    g = guarded()
    g.run('stand_in', 'ppi', (x, out, 33), entry)
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    (v,) = ei.value.violations
    assert (v['entry'], v['kind'], v['args'], v['side'], v['count'], v['first'], v['last']) == \
        ('stand_in', 'band', (1,), where, 1, 0, 0)
    assert v['scalars'] == {2: 33} and 'stand_in' in str(ei.value) and '33' in str(ei.value)
    assert (out == 5).all()                       # the interior still came back


def test_a_changed_byte_in_the_last_band_word_is_caught():
    out = torch.zeros(16)

    def entry(args):
        (o,) = args
        w = _raw_words(o, 16 + G.BAND_WORDS - 1, 16 + G.BAND_WORDS)
        w.view(torch.uint8)[3] ^= 1               # one bit of the most significant byte of the last word of the band
        w2 = _raw_words(o, 16 + 5, 16 + 6)
        w2.view(torch.uint8)[0] += 1

    g = guarded()
    g.run('stand_in', 'p', (out,), entry)
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    (v,) = ei.value.violations
    assert (v['side'], v['count'], v['first'], v['last']) == ('behind', 2, 20, 4 * (G.BAND_WORDS - 1))


def test_overlapping_views_are_one_group_and_see_each_other():
    buf = torch.zeros(64)
    a, b, c = buf[:40], buf[24:64], torch.zeros(8)
    assert [idx for _, _, idx in G.group_ranges([(0, 160), (96, 256), (256, 300), (1000, 1004)])] == [[0, 1], [2], [3]]

    def entry(args):
        x, y, z = args
        assert y.data_ptr() - x.data_ptr() == 24 * 4          # the same layout as the originals
        x[30] = 7.0                                           # = y[6]
        assert y[6] == 7.0
        y[39] = 9.0
        z.fill_(1.0)

    with guarded(replay=True) as g:
        g.run('stand_in', 'ppp', (a, b, c), entry)
    assert buf[30] == 7.0 and b[6] == 7.0 and buf[63] == 9.0 and (c == 1).all()
    assert buf.sum() == 16.0


def test_touching_views_stay_apart_so_an_overrun_into_the_neighbour_shows():
    buf = torch.zeros(64)
    a, b = buf[:32], buf[32:]

    def entry(args):
        x, y = args
        assert y.data_ptr() - x.data_ptr() != 32 * 4
        _raw_words(x, 32, 33).fill_(1)

    g = guarded()
    g.run('stand_in', 'pp', (a, b), entry)
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    assert [(v['args'], v['side'], v['first']) for v in ei.value.violations] == [((0,), 'behind', 0)]


@pytest.mark.parametrize('offset', [0, 4, 8, 16, 252])
def test_interior_keeps_the_pointer_modulo_256(offset):
    base = torch.zeros(1024 + 64)
    lead = (-base.data_ptr()) % 256 // 4                      # first 256-byte aligned element
    t = base[lead + offset // 4: lead + offset // 4 + 100]
    assert t.data_ptr() % 256 == offset
    seen = []

    def entry(args):
        seen.append(args[0].data_ptr())

    with guarded(replay=True) as g:
        g.run('stand_in', 'p', (t,), entry)
    assert len(seen) == 2 and all(p % 256 == offset and p != t.data_ptr() for p in seen)


def test_replay_catches_a_result_that_depends_on_the_band():
    x, out = torch.ones(8), torch.zeros(8)

    def entry(args):
        a, o = args
        o.copy_(a)
        o[7] = _raw_words(a, 8, 9).view(torch.float32)[0]     # reads one word past its input

    g = guarded(replay=True)
    g.run('stand_in', 'pp', (x, out), entry)
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    (v,) = ei.value.violations
    assert (v['kind'], v['args'], v['count'], v['first']) == ('replay', (1,), 1, 28)


def test_replay_starts_from_the_pre_call_contents():
    acc = torch.ones(4)

    def entry(args):
        args[0].add_(1.0)                                     # in place: a second run from the POST-call state would give 3

    with guarded(replay=True) as g:
        g.run('stand_in', 'p', (acc,), entry)
    assert (acc == 2).all()


def test_error_code_is_raised_after_the_check_and_a_rejected_call_must_not_write():
    out = torch.zeros(8)

    def reject(args):
        raise RuntimeError('hipError_t 1')

    def reject_dirty(args):
        args[0][3] = 1.0
        raise RuntimeError('hipError_t 1')

    with guarded(replay=True) as g:
        with pytest.raises(RuntimeError, match='hipError_t 1'):
            g.run('stand_in', 'pi', (out, 8), reject)
    assert (out == 0).all()
    g = guarded()
    with pytest.raises(RuntimeError, match='hipError_t 1'):
        g.run('stand_in', 'pi', (out, 8), reject_dirty)
    with pytest.raises(G.GuardViolation) as ei:
        g.check()
    (v,) = ei.value.violations
    assert (v['kind'], v['args'], v['count'], v['first']) == ('rejected', (0,), 1, 12)


def test_call_hook_is_looked_up_at_call_time_and_restored():
    from tvae import _lib
    assert _lib.CALL_HOOK is None
    with G.GuardedCalls() as g:
        assert _lib.CALL_HOOK == g.run
        with G.GuardedCalls() as inner:
            assert _lib.CALL_HOOK == inner.run
        assert _lib.CALL_HOOK == g.run
    assert _lib.CALL_HOOK is None
