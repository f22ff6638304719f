"""The negative control of tests/padded.py, on the CPU: a word written one element before or one
element after a padded operand makes fetch() report it, for every dtype, fill and offset; writes
inside the operand do not."""
import numpy as np
import pytest

import padded

_FILLS = {np.int8: [padded.FILL_A, padded.FILL_B], np.int16: [padded.FILL_A, padded.FILL_B],
          np.int32: [padded.FILL_A, padded.FILL_B], np.float32: [padded.NAN_FILL, padded.F32_SENTINEL]}


@pytest.mark.parametrize("dt", list(_FILLS), ids=lambda d: np.dtype(d).name)
def test_padded_reports_a_write_outside_the_operand(dt):
    import torch
    for fill in _FILLS[dt]:
        for o in (0, 1, 2, 3, 4, 8):
            data = np.arange(1, 3 * 7 + 1).astype(dt).reshape(3, 7)
            p = padded.Padded(torch, dt, (3, 7), o, fill, device="cpu").put(torch, data)
            assert p.ptr % 16 == (o * np.dtype(dt).itemsize) % 16
            got, ok = p.fetch()
            assert ok and got.tobytes() == data.tobytes() and got.dtype == dt
            p.t[0, 0] = 9                                  # inside: first and last word
            p.t[2, 6] = 9
            assert p.fetch()[1]
            for at, name in ((p.lo - 1, "before"), (p.hi, "after"), (0, "first pad word"),
                             (p.hi + padded.PAD - 1, "last pad word")):
                q = padded.Padded(torch, dt, (3, 7), o, fill, device="cpu").put(torch, data)
                q.flat[at] = 1
                got, ok = q.fetch()
                assert not ok, (fill, o, name)
                assert got.tobytes() == data.tobytes()
            p.reset()
            got, ok = p.fetch()
            assert ok and (got.view(padded._BITS[np.dtype(dt).itemsize]) == p.word).all()


def test_padded_fills():
    """0x55.. / 0xAA.. per width; the f32 input fill is a NaN and the f32 sentinel is finite."""
    assert padded.fill_word(np.int8, padded.FILL_A) == 0x55
    assert padded.fill_word(np.int16, padded.FILL_B) == np.int16(-0x5556)
    assert padded.fill_word(np.int32, padded.FILL_A) == 0x55555555
    import torch
    for fill, nan in ((padded.NAN_FILL, True), (padded.F32_SENTINEL, False)):
        p = padded.Padded(torch, np.float32, 4, 1, fill, device="cpu")
        got, ok = p.fetch()
        assert ok and bool(np.isnan(got).all()) == nan and bool(np.isfinite(got).all()) != nan
