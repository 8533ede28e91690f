"""CPU: the one launch path into the library.  _lib.call makes the operands' device current (a guard only when it is not), hands
over that device's stream, then the options, the launcher and the error query - against a recording stand-in for the library."""
import types

import pytest
import torch

from stratified_transformer_amd import _lib, pointops2_cuda

CURRENT = 0


class FakeLibrary:
    """Every entry point is callable and notes (name, args) in `log`; pointops2_last_error answers `error`."""

    def __init__(self, log, error=None):
        self.log, self.error = log, error

    def __getattr__(self, name):
        def entry(*args):
            self.log.append((name, args))
            return self.error if name == "pointops2_last_error" else None
        return entry


@pytest.fixture
def launch(monkeypatch):
    """-> (log, set_error): the library, the current-device query, torch.cuda.device and the stream getter replaced by recorders"""
    log = []
    fake = FakeLibrary(log)

    class Guard:
        def __init__(self, device):
            self.device = device
            log.append(("guard built", (device,)))

        def __enter__(self):
            log.append(("guard entered", (self.device,)))

        def __exit__(self, *exc):
            log.append(("guard left", (self.device,)))
            return False

    def no_torch_stream(device=None):
        raise AssertionError("torch.cuda.current_stream was asked for a device with an index")
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "_current_device", lambda: CURRENT)
    monkeypatch.setattr(_lib, "_raw_stream", lambda index: 1000 + index)
    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(torch.cuda, "current_stream", no_torch_stream)
    return log, lambda message: setattr(fake, "error", message)


def names(log):
    return [name for name, _ in log]


def test_current_device_launches_without_a_guard(launch):
    log, _ = launch
    before = _lib.CALLS[0]
    _lib.call("some_launcher", 1, 2.5, None, device=torch.device("cuda", CURRENT))
    assert log == [("pointops2_set_stream", (1000 + CURRENT,)), ("some_launcher", (1, 2.5, None)), ("pointops2_last_error", ())]
    assert _lib.CALLS[0] == before + 1


def test_another_device_runs_the_whole_sequence_under_its_guard(launch):
    log, _ = launch
    other = torch.device("cuda", CURRENT + 1)
    before = _lib.CALLS[0]
    _lib.call("some_launcher", 7, device=other)
    assert log == [("guard built", (other,)), ("guard entered", (other,)), ("pointops2_set_stream", (1000 + CURRENT + 1,)),
                   ("some_launcher", (7,)), ("pointops2_last_error", ()), ("guard left", (other,))]
    assert _lib.CALLS[0] == before + 1


@pytest.mark.parametrize("index", [CURRENT, CURRENT + 1])
def test_options_go_between_the_stream_and_the_launcher(launch, index):
    log, _ = launch
    opts = _lib.LaunchOpts(table_rows=31)
    _lib.call("some_launcher", 3, device=torch.device("cuda", index), opts=opts)
    calls = [entry for entry in log if not entry[0].startswith("guard")]
    assert calls == [("pointops2_set_stream", (1000 + index,)), ("pointops2_set_launch_opts", (opts,)), ("some_launcher", (3,)),
                     ("pointops2_last_error", ())]
    assert calls[1][1][0] is opts
    del log[:]
    _lib.call("some_launcher", 3, device=torch.device("cuda", index), opts=None)
    assert "pointops2_set_launch_opts" not in names(log)


@pytest.mark.parametrize("index", [CURRENT, CURRENT + 1])
def test_a_library_error_is_raised_with_the_launchers_name(launch, index):
    log, set_error = launch
    set_error(b"d != 16 and d != 32")
    before = _lib.CALLS[0]
    with pytest.raises(RuntimeError) as raised:
        _lib.call("some_launcher", device=torch.device("cuda", index))
    assert str(raised.value) == "some_launcher: d != 16 and d != 32"
    assert _lib.CALLS[0] == before + 1
    if index == CURRENT:
        assert not any(name.startswith("guard") for name in names(log))
    else:  # the guard is left all the same, after the error query
        assert names(log)[:2] == ["guard built", "guard entered"] and names(log)[-2:] == ["pointops2_last_error", "guard left"]


def test_no_device_or_no_index_means_the_current_device(launch, monkeypatch):
    log, _ = launch
    asked = []

    def current_stream(device=None):
        asked.append(device)
        return types.SimpleNamespace(cuda_stream=77)

    def no_query():
        raise AssertionError("the current device was queried though no index was given")
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(_lib, "_current_device", no_query)
    before = _lib.CALLS[0]
    for device in (None, torch.device("cuda")):
        del log[:]
        _lib.call("some_launcher", 5, device=device)
        assert log == [("pointops2_set_stream", (77,)), ("some_launcher", (5,)), ("pointops2_last_error", ())]
    assert asked == [None, torch.device("cuda")]
    assert _lib.CALLS[0] == before + 2


def test_the_extension_modules_call_forwards_to_the_one_path(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda *args, **kwargs: seen.append((args, kwargs)))
    ref = types.SimpleNamespace(device=torch.device("cuda", 3))
    opts = _lib.LaunchOpts()
    pointops2_cuda._call("x", ref, 1, 2, opts=opts)
    assert seen == [(("x", 1, 2), {"device": ref.device, "opts": opts})]
    assert seen[0][1]["opts"] is opts
    assert pointops2_cuda._chk is _lib.check_tensors


def test_check_tensors_checks_each_triple_in_order():
    with pytest.raises(RuntimeError, match="^b: expected a GPU tensor"):
        _lib.check_tensors((torch.zeros(2), torch.float32, "b"), (torch.zeros(2), torch.int32, "c"))
    _lib.check_tensors()
