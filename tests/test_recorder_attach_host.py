"""Host tests of what the recorders share in front of the library: the agreement of the ranks of a partition
(knpemi.recording.agree_across_ranks), the one attach path of DeviceStepper and the refusals of partitioned steps that
it leaves on the taps, and the table of tools/recorder_cost.py.  Stub recorders and a stub library: nothing is loaded."""
import importlib.util
import os
import types
from unittest import mock

import pytest

from knpemi.recording import Tap, agree_across_ranks
from knpemi.stepper import DeviceStepper

FIELDS = ("watches", "every", "capacity")


def test_ranks_that_agree_pass():
    mine = dict(watches=[(1, 7)], every=2, capacity=8, other=0)
    agree_across_ranks([dict(mine), dict(mine, other=1), dict(mine)], FIELDS, "flux recorders", "advice")


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("what,value", [("watches", [(1, 3)]), ("every", 3), ("capacity", 9)])
def test_a_differing_field_names_the_field_and_the_rank(what, value, rank):
    mine = dict(watches=[(1, 7)], every=2, capacity=8)
    allr = [dict(mine) for _ in range(3)]
    allr[rank][what] = value
    with pytest.raises(ValueError) as e:
        agree_across_ranks(allr, FIELDS, "flux recorders", "every rank must watch the same sub-domains")
    assert str(e.value) == (f"flux recorders differ between ranks: {what} of rank {rank} is {value!r}, of rank 0 "
                            f"{mine[what]!r} (every rank must watch the same sub-domains)")


# the texts DeviceStepper.step(halo) raised before the taps carried them
REFUSALS = dict(
    observe="observables attached without a halo are not recorded on partitioned steps: pass halo= to DeviceStepper.observe",
    fluxes="ion fluxes attached without a halo are not recorded on partitioned steps (a rank's sums would include its ghost "
           "cells): pass halo= to DeviceStepper.fluxes",
    exchange="a membrane exchange attached without a halo is not recorded on partitioned steps (a rank's sums would include "
             "its ghost facets): pass halo= to DeviceStepper.exchange",
    track="field maps with a series watch are not recorded on partitioned steps (a rank's sums would include its ghost "
          "items): track maps without series=True",
    monitor="membrane monitors are not recorded on partitioned steps (a rank's reductions would include its ghost dofs): "
            "run DeviceStepper.monitor on one rank")


def _stepper():
    """A stepper without a device problem: what the attach methods and the head of step() touch."""
    st = object.__new__(DeviceStepper)
    st.dp, st.lib, st.taps, st.dt = mock.MagicMock(), mock.MagicMock(), {}, 1e-4
    return st


def _recorder(**kw):
    return mock.MagicMock(_drain=None, n_cols=3, **kw)


def test_partitioned_steps_are_refused_through_the_taps():
    st = _stepper()
    halo, other = types.SimpleNamespace(dp=st.dp), types.SimpleNamespace(dp=st.dp)
    st.observe(_recorder(), halo=halo)
    st.detect(_recorder())
    st.fluxes(_recorder())
    st.exchange(_recorder(), halo=halo)
    st.track(_recorder(has_series=True))
    st.monitor(_recorder())
    assert list(st.taps) == ["observe", "detect", "fluxes", "exchange", "track", "monitor"]
    assert [st.taps[n].halo for n in st.taps] == [halo, None, None, halo, None, None]
    assert st.taps["detect"].partition_refusal is None
    assert {n: st.taps[n].partition_refusal for n in REFUSALS} == REFUSALS
    for tap in st.taps.values():
        tap.refuse_partitioned(None)             # steps without a halo: nothing is refused
    # with the halo of observe and exchange the first tap to refuse is the fluxes', then the maps', then the monitor's
    for name in ("fluxes", "track", "monitor"):
        with pytest.raises(NotImplementedError) as e:
            st.step(halo)
        assert str(e.value) == REFUSALS[name]
        del st.taps[name]
    for tap in st.taps.values():
        tap.refuse_partitioned(halo)
    # another halo than the one attached with
    for name in ("observe", "exchange"):
        with pytest.raises(NotImplementedError) as e:
            st.step(other)
        assert str(e.value) == REFUSALS[name]
        del st.taps[name]
    st.taps["detect"].refuse_partitioned(other)


def test_maps_without_a_series_need_no_halo():
    st = _stepper()
    st.track(_recorder(has_series=False))
    assert st.taps["track"].partition_refusal is None and st.taps["track"].read is None


def test_the_attach_path_checks_before_it_sets_up():
    st = _stepper()
    rec = _recorder()
    for attach in (st.observe, st.fluxes, st.exchange, st.track, st.monitor):
        for kw in (dict(every=0), dict(capacity=0)):
            with pytest.raises(ValueError, match="every and capacity must be positive"):
                attach(rec, **kw)
    with pytest.raises(ValueError, match="every must be positive"):
        st.detect(rec, every=0)
    with pytest.raises(ValueError, match=r"fluxes\(halo=...\): attach the halo to this stepper's problem first"):
        st.fluxes(rec, halo=types.SimpleNamespace(dp=None))
    assert not st.taps and not rec._attach.called and not rec.upload.called
    busy = dict(detect="membrane events", fluxes="ion fluxes", exchange="a membrane exchange", track="field maps",
                monitor="membrane monitors")
    for name, what in busy.items():
        getattr(st, name)(_recorder())
        with pytest.raises(RuntimeError, match=f"this stepper records {what} already"):
            getattr(st, name)(_recorder())
    st.taps.clear()
    attached = dict(observe="these observables are", fluxes="these fluxes are", exchange="this exchange is",
                    track="these maps are", monitor="this monitor is")
    for name, what in attached.items():
        with pytest.raises(RuntimeError, match=f"{what} attached to a stepper already"):
            getattr(st, name)(mock.MagicMock(_drain=lambda: None))
    assert not st.taps


def test_a_failed_hook_is_raised_in_place_of_the_status():
    st = _stepper()
    st.lib.knpemi_flux_record.return_value = 5
    halo = types.SimpleNamespace(dp=st.dp, _hook_error=KeyError("in the hook"))
    st.fluxes(_recorder(), halo=halo)
    with pytest.raises(KeyError, match="in the hook"):
        st.taps["fluxes"].tick(1, st.dt)
    assert isinstance(st.taps["fluxes"], Tap) and st.taps["fluxes"].keep is not None


def test_recorder_cost_covers_the_six_recorders():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "recorder_cost.py")
    spec = importlib.util.spec_from_file_location("recorder_cost", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    names = {"observe", "events", "fluxes", "exchange", "maps", "monitor"}
    assert set(tool.RECORDERS) == set(tool.KERNEL) == names
    ap = tool.parser()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(["--help"])
    assert e.value.code == 0
    for name in names:
        args = ap.parse_args(["--recorder", name, "--repeats", "5"])
        assert (args.recorder, args.workload, args.steps, args.warmup, args.repeats, args.stats) == (name, "config2", 200, 20, 5, None)
    with pytest.raises(SystemExit):
        ap.parse_args(["--recorder", "fields"])
