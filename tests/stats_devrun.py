"""Device-resident requests of the four statistics entries (test helper, in the style of devrun.py).

`DeviceEstep`, `DeviceDrawStats`, `DeviceDrawStatsGauss` and `DeviceExpect`
take the same arguments as hhmm_amd.estep / draw_stats / draw_stats_gauss /
expected_stats, copy the inputs to the GPU once (hhmm_amd._stats.DeviceStats:
NaN outputs, status -1) and run the entry's _device function on torch's stream
with device-side outputs.  `stats()` returns them in the host entry's layout.
"""
import sys

import torch

import hhmm_amd  # noqa: F401
from hhmm_amd._stats import DeviceStats

_estep = sys.modules["hhmm_amd.estep"]
_gibbs = sys.modules["hhmm_amd.gibbs"]
_gg = sys.modules["hhmm_amd.gibbs_gauss"]


class _Device:
    def __init__(self, lib, entry, prepared):
        pr, res, out = prepared
        self.dv = DeviceStats(lib, entry, pr, res, {name: a.shape for name, a in out.items()})

    def run(self):
        st = self.dv.run()
        torch.cuda.synchronize()
        return st

    def stats(self):
        return self.dv.stats()


class DeviceEstep(_Device):
    def __init__(self, lib, model, data, draws, pairing="grid"):
        super().__init__(lib, "estep", _estep.prepare(model, data, draws, pairing))


class DeviceDrawStats(_Device):
    def __init__(self, lib, model, data, draws, uniforms, pairing="grid"):
        super().__init__(lib, "draw_stats", _gibbs.prepare(model, data, draws, uniforms, pairing))


class DeviceDrawStatsGauss(_Device):
    def __init__(self, lib, data, draws, uniforms, pairing="grid"):
        super().__init__(lib, "draw_stats_gauss", _gg.prepare(data, draws, uniforms, pairing))


class DeviceExpect(_Device):
    def __init__(self, lib, model, data, draws, pairing="grid"):
        super().__init__(lib, "expected_stats", _gibbs._request(model, data, draws, pairing, -1))
