"""model/expert_towers.py: which of the five ways the E expert towers run.  `choose_path` is held to the table over the full product
of its inputs; no tensor, no GPU.

    1. grouped switch on and experts eligible                                          -> grouped
       (switch on, not eligible: ONE warning per process, then on down the table)
    2. frozen, pixels on the device, MM_MOE_GRAPH != "0"                                -> frozen_graph
    3. not frozen, pixels on the device and without grad, MM_MOE_GRAPH != "0",
       MM_MOE_TRAIN_GRAPH != "0", every trainable parameter flat-backed                 -> train_graph
       (the graphs may decline a call: then rule 4 decides it)
    4. one expert, or pixels off the device, or MM_MOE_STREAMS == "0"                   -> serial, otherwise streams"""
import itertools
import warnings

import pytest

from multimeditron_amd.model import expert_towers as T

FACTS = ("grouped_on", "eligible", "on_device", "frozen", "pixels_need_grad", "graphable", "graph", "train_graph", "streams")


def product():
    for bits in itertools.product([False, True], repeat=len(FACTS)):
        for E in (1, 3):
            yield dict(zip(FACTS, bits), E=E)


def eager(f):
    return "serial" if f["E"] == 1 or not f["on_device"] or not f["streams"] else "streams"


def expected(f):
    """the table above, first match wins"""
    if f["grouped_on"] and f["eligible"]:
        return "grouped"
    if f["frozen"] and f["on_device"] and f["graph"]:
        return "frozen_graph"
    if not f["frozen"] and f["on_device"] and not f["pixels_need_grad"] and f["graph"] and f["train_graph"] and f["graphable"]:
        return "train_graph"
    return eager(f)


class Calls:
    """the lazily evaluated facts, and how often each was asked for"""

    def __init__(self, f):
        self.f, self.n = f, {"ineligible": 0, "frozen": 0, "graphable": 0}

    def ask(self, what, value):
        def fn():
            self.n[what] += 1
            return value
        return fn

    def choose(self):
        f, on = self.f, lambda flag: "1" if flag else "0"
        return T.choose_path(f["grouped_on"], self.ask("ineligible", None if f["eligible"] else "the experts' vision configs differ"),
                             f["on_device"], self.ask("frozen", f["frozen"]), f["pixels_need_grad"], self.ask("graphable", f["graphable"]),
                             f["E"], graph=on(f["graph"]), train_graph=on(f["train_graph"]), streams=on(f["streams"]))


def test_the_chooser_follows_the_table(monkeypatch):
    monkeypatch.setattr(T, "_warned_ineligible", True)               # the warning has its own test
    seen = set()
    for f in product():
        c = Calls(f)
        path = c.choose()
        assert path == expected(f), f
        seen.add(path)
        assert c.n["ineligible"] == (1 if f["grouped_on"] else 0), f              # asked only when the switch is on
        assert c.n["frozen"] == (0 if path == "grouped" else 1), f                # walks every parameter: not on the grouped path
        assert c.n["graphable"] <= 1, f
    assert seen == {"grouped", "frozen_graph", "train_graph", "serial", "streams"}


def test_a_declined_graph_call_takes_the_eager_rule(monkeypatch):
    """_trainable_towers may decline a call (a forward of that pixel shape still awaits its backward): rule 4 decides that call"""
    monkeypatch.setattr(T, "_warned_ineligible", True)
    n = 0
    for f in product():
        if Calls(f).choose() != "train_graph":
            continue
        n += 1
        assert f["on_device"] and not f["frozen"]
        assert T.eager_path(f["E"], True, "1" if f["streams"] else "0") == ("serial" if f["E"] == 1 or not f["streams"] else "streams"), f
    assert n > 0


@pytest.mark.parametrize("value,on", [("1", True), ("0", False), ("", True), ("yes", True)])
def test_a_switch_is_off_only_at_zero(monkeypatch, value, on):
    """MM_MOE_GRAPH / MM_MOE_TRAIN_GRAPH / MM_MOE_STREAMS: anything but "0" leaves the path on"""
    monkeypatch.setattr(T, "_warned_ineligible", True)
    choose = lambda frozen, **kw: T.choose_path(False, lambda: None, True, lambda: frozen, False, lambda: True, 3, **kw)
    assert choose(True, graph=value) == ("frozen_graph" if on else "streams")
    assert choose(False, graph=value) == ("train_graph" if on else "streams")
    assert choose(False, train_graph=value) == ("train_graph" if on else "streams")
    assert choose(False, train_graph="0", streams=value) == ("streams" if on else "serial")


def test_the_switches_are_read_from_the_environment_per_call(monkeypatch):
    for k in ("MM_MOE_GRAPH", "MM_MOE_TRAIN_GRAPH", "MM_MOE_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    assert T._switches() == ("1", "1", "1")
    monkeypatch.setenv("MM_MOE_GRAPH", "0")
    monkeypatch.setenv("MM_MOE_STREAMS", "")
    assert T._switches() == ("0", "1", "")
    monkeypatch.setenv("MM_MOE_TRAIN_GRAPH", "0")
    assert T._switches() == ("0", "0", "")


def test_ineligible_experts_warn_once_per_process(monkeypatch):
    monkeypatch.setattr(T, "_warned_ineligible", False)
    why = "the experts' dtypes differ"
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        paths = [T.choose_path(True, lambda: why, True, lambda: False, False, lambda: True, 3) for _ in range(3)]
        paths.append(T.choose_path(False, lambda: why, True, lambda: False, False, lambda: True, 3))
    assert paths == ["train_graph"] * 4                                       # on down the table
    said = [str(w.message) for w in got if "grouped_towers" in str(w.message)]
    assert said == [f"grouped_towers: {why}; the expert towers run one by one"]
    assert T._warned_ineligible is True


def test_run_experts_runs_a_declined_call_eagerly(monkeypatch):
    """the wiring behind the table, on stand-ins: the graphs decline, the call runs one tower after the other, `post` after each"""
    from types import SimpleNamespace as NS
    log = []

    class Hidden:
        shape = (2, 5, 4)

        def reshape(self, *shape):
            return self

    class Expert:
        def __init__(self, i):
            self.i = i

        def parameters(self):
            return [NS(requires_grad=True, _mm_flat=object())]

        def __call__(self, px):
            log.append(("tower", self.i))
            return NS(last_hidden_state=Hidden())

    monkeypatch.setattr(T, "_warned_ineligible", True)
    monkeypatch.setattr(T, "_trainable_towers", lambda experts, pixels, tower: log.append("declined"))      # -> None
    monkeypatch.setattr(T.Fm, "drop_cls", lambda x, n, tokens: "tokens")
    monkeypatch.delenv("MM_MOE_GROUPED", raising=False)
    monkeypatch.delenv("MM_MOE_GRAPH", raising=False)
    monkeypatch.delenv("MM_MOE_TRAIN_GRAPH", raising=False)
    monkeypatch.setenv("MM_MOE_STREAMS", "0")
    pixels = NS(shape=(2, 3, 8, 8), is_cuda=True, requires_grad=False)
    outs = T.run_experts([Expert(i) for i in range(3)], pixels, post=lambda e, o: log.append(("post", e)) or (e, o))
    assert outs == [(0, "tokens"), (1, "tokens"), (2, "tokens")]
    assert log == ["declined", ("tower", 0), ("post", 0), ("tower", 1), ("post", 1), ("tower", 2), ("post", 2)]
