"""What the GPU tests of the stage timing getters share: one call made with timing on and once more with timing off,
and the rule every stage's ``last_timing`` keeps (ovl_last_timing)."""


def timed_and_untimed(engine, call, last=None):
    """``call()`` with timing on, then with timing off.  Returns the two results and, for each, ``last_timing()``
    merged with ``last()`` (a stage's own getter) where one is given."""
    def stats():
        out = dict(engine.last_timing())
        if last is not None:
            out.update(last())
        return out
    engine.set_timing(True)
    try:
        got_on = call()
        on = stats()
    finally:
        engine.set_timing(False)
    got_off = call()
    return got_on, on, got_off, stats()


def assert_kernel_inside_call(on, off):
    """Timing on: 0 < kernel_ms <= call_ms.  Timing off: kernel_ms is 0.0 and the call is still clocked."""
    assert 0.0 < on["kernel_ms"] <= on["call_ms"], on
    assert off["kernel_ms"] == 0.0 and off["call_ms"] > 0.0, off
