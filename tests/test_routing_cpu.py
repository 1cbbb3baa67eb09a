"""The routing rule at its thresholds, without a GPU: a stage called with ``device=None`` (``form="auto"``) takes the
device form iff its work reaches the stage's threshold and a device can serve it -- an engine was given, or
``device_count() > 0`` -- and the count is not asked for when the threshold fails or an engine was given (on a box
without a GPU the count loads the library, which small inputs must not pay for).

The rule is asserted twice.  Through ``correct._use_device``, which was a function before the rule had one home, so
those tests ran unchanged on the commit before ``engine.use_device``; and on ``use_device`` itself, for what only its
signature can show (a callable ``work``).  Then each of the eight entry points that route by the rule, on inputs of one
or two reads of 8 bases: ``device=None`` returns what ``device=False`` returns, with ``device_count`` made to raise
wherever the threshold alone decides."""
import networkx as nx
import numpy as np
import pytest

from ovlgraph import consensus, correct, engine, layout, overlapGraphs, performanceMeasures

MIN = 5
FORM = {None: "auto", True: "device", False: "host"}
ENGINE = object()  # stands in for an engine: the rule only asks whether one was given
READS = ["ACGTTGCA", "TGCAATGC"]
CONTIGS = ["ACGTTGCAATGC"]


def _decide(monkeypatch, device, work, eng):
    """The rule with threshold MIN through read correction's site (its own threshold is 0)."""
    monkeypatch.setattr(correct, "CORRECT_DEVICE_MIN_WINDOWS", MIN)
    return correct._use_device(FORM[device], eng, work)


def _count(n):
    return lambda: n


def _no_count():
    raise AssertionError("device_count() was called")


@pytest.mark.parametrize("work", [0, MIN - 1, MIN, 10 ** 12])
def test_a_forced_choice_comes_back_whatever_the_work(monkeypatch, work):
    monkeypatch.setattr(engine, "device_count", _no_count)
    for eng in (None, ENGINE):
        assert _decide(monkeypatch, True, work, eng) is True
        assert _decide(monkeypatch, False, work, eng) is False


def test_the_threshold_is_inclusive_with_an_engine(monkeypatch):
    monkeypatch.setattr(engine, "device_count", _no_count)
    assert _decide(monkeypatch, None, MIN - 1, ENGINE) is False
    assert _decide(monkeypatch, None, MIN, ENGINE) is True


def test_without_an_engine_the_device_count_decides(monkeypatch):
    monkeypatch.setattr(engine, "device_count", _count(0))
    assert _decide(monkeypatch, None, MIN, None) is False
    monkeypatch.setattr(engine, "device_count", _count(1))
    assert _decide(monkeypatch, None, MIN, None) is True
    assert _decide(monkeypatch, None, MIN - 1, None) is False


def test_the_device_count_is_not_asked_for_below_the_threshold_or_with_an_engine(monkeypatch):
    monkeypatch.setattr(engine, "device_count", _no_count)
    assert _decide(monkeypatch, None, MIN - 1, None) is False
    assert _decide(monkeypatch, None, MIN, ENGINE) is True
    with pytest.raises(AssertionError):  # (and at the threshold without an engine it is)
        _decide(monkeypatch, None, MIN, None)


def test_use_device_itself(monkeypatch):
    use_device = engine.use_device
    monkeypatch.setattr(engine, "device_count", _no_count)

    def never():
        raise AssertionError("work was evaluated")
    for eng in (None, ENGINE):
        assert use_device(True, never, MIN, eng) is True and use_device(False, never, MIN, eng) is False
        assert use_device(True, 0, MIN, eng) is True and use_device(False, 10 ** 12, MIN, eng) is False
    assert use_device(None, MIN - 1, MIN, ENGINE) is False and use_device(None, MIN, MIN, ENGINE) is True
    assert use_device(None, lambda: MIN - 1, MIN, None) is False
    assert use_device(None, lambda: MIN, MIN, ENGINE) is True
    with pytest.raises(AssertionError):
        use_device(None, MIN, MIN, None)
    monkeypatch.setattr(engine, "device_count", _count(0))
    assert use_device(None, MIN, MIN, None) is False
    monkeypatch.setattr(engine, "device_count", _count(2))
    assert use_device(None, lambda: MIN, MIN, None) is True and use_device(None, MIN - 1, MIN, None) is False


# ---------------------------------------------------------------- the eight entry points
def _same(x, y):
    """Equal results, field for field: arrays by value and dtype, graphs by their ordered edges with data."""
    assert type(x) is type(y)
    if isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    elif isinstance(x, dict):
        assert list(x) == list(y)
        for k in x:
            _same(x[k], y[k])
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y)
        for a, b in zip(x, y):
            _same(a, b)
    elif isinstance(x, nx.DiGraph):
        assert list(x.nodes()) == list(y.nodes())
        assert list(x.edges(data=True)) == list(y.edges(data=True))
    elif isinstance(x, (consensus.Pileup, performanceMeasures.ReadDepth)):
        _same(vars(x), vars(y))
    else:
        assert x == y


def _triangle():
    G = nx.DiGraph()
    G.add_edge("ACGTTGCA", "GTTGCAAT", weight=6, end_position=6)
    G.add_edge("ACGTTGCA", "TGCAATGC", weight=4, end_position=4)
    G.add_edge("GTTGCAAT", "TGCAATGC", weight=6, end_position=6)
    return G


ENTRY_POINTS = {
    # consensus._place and consensus.pileup: the placement comes from read_best, then the pileup
    "polish_contigs": lambda d: consensus.polish_contigs(CONTIGS, READS, 8, min_depth=1, device=d),
    "pileup": lambda d: consensus.pileup(CONTIGS, READS, 8, place=[0, 0], min_depth=1, device=d),
    "pileup_placed": lambda d: consensus.pileup_placed(CONTIGS, READS, [0, 0], [0, 4], min_depth=1, device=d),
    "layout": lambda d: layout.layout(READS, [0], [1], [40], [4], device=d),
    "read_depth": lambda d: performanceMeasures.read_depth(CONTIGS, READS, 8, device=d,
                                                           rng=np.random.RandomState(0)),
    "transitive_reduction": lambda d: overlapGraphs.transitive_reduction(_triangle(), device=d),
    "transitive_reduction2": lambda d: overlapGraphs.transitive_reduction2(_triangle(), device=d),
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_small_inputs_take_the_host_form_and_never_ask_for_the_count(monkeypatch, name):
    host = ENTRY_POINTS[name](False)
    monkeypatch.setattr(engine, "device_count", _no_count)
    _same(ENTRY_POINTS[name](None), host)


def test_read_correction_auto_is_its_host_form_without_a_device(monkeypatch):
    """The eighth: its threshold is 0 windows, so the count decides; without a device "auto" is "host"."""
    monkeypatch.setattr(engine, "device_count", _count(0))
    _same(correct.kmer_spectrum(READS, 4), correct.kmer_spectrum(READS, 4, form="host"))
    _same(correct.correct_reads(READS, 4, 1), correct.correct_reads(READS, 4, 1, form="host"))


def test_the_small_inputs_do_something():
    assert ENTRY_POINTS["layout"](False)["contigs"] == ["ACGTTGCAATGC"]
    assert ENTRY_POINTS["pileup_placed"](False).called == CONTIGS
    assert ENTRY_POINTS["read_depth"](False).coverage[CONTIGS[0]].tolist() == [1] * 4 + [2] * 4 + [1] * 4
    assert ENTRY_POINTS["transitive_reduction"](False).number_of_edges() == 2
    assert ENTRY_POINTS["transitive_reduction2"](False).number_of_edges() == 2
