"""Device-resident Gaussian draw-statistics requests (test helper, in the style of draw_stats_devrun.py).

`DeviceDrawStatsGauss` takes the same (data, draws, uniforms) as
hhmm_amd.draw_stats_gauss, copies the inputs to the GPU once and runs
hhmm_draw_stats_gauss_device on torch's stream with device-side outputs.
`stats()` returns them in hhmm_amd.draw_stats_gauss's host layout.
"""
import ctypes as C
import sys

import numpy as np
import torch

import hhmm_amd  # noqa: F401

_gg = sys.modules["hhmm_amd.gibbs_gauss"]


class DeviceDrawStatsGauss:
    def __init__(self, lib, data, draws, uniforms, pairing="grid"):
        self.lib = lib
        self.dev = torch.device("cuda", torch.cuda.current_device())
        pr, res, out = _gg.prepare(data, draws, uniforms, pairing)
        self._keep = {}
        for arr in pr.keep:
            self._keep[arr.ctypes.data] = torch.from_numpy(np.asarray(arr).reshape(-1, order="F").copy()).to(self.dev)
        for struct in (pr.req.data, pr.req.draws):
            for name, ctype in struct._fields_:
                v = getattr(struct, name)
                if ctype is C.c_void_p and v and v in self._keep:
                    setattr(struct, name, self._keep[v].data_ptr())
        pr.req.ffbs_u = self._keep[pr.req.ffbs_u].data_ptr()
        self.shapes = {name: a.shape for name, a in out.items()}
        self.out = {}
        for name, shape in self.shapes.items():
            self.out[name] = torch.full((int(np.prod(shape)),), float("nan"), dtype=torch.float64, device=self.dev)
            setattr(res, name, self.out[name].data_ptr())
        self.status = torch.full((pr.P,), -1, dtype=torch.int32, device=self.dev)
        res.pair_status = self.status.data_ptr()
        ws = C.c_size_t(0)
        assert lib.hhmm_draw_stats_gauss_workspace_size(C.byref(pr.req), C.byref(ws)) == 0
        self.ws = torch.empty(max(int(ws.value), 256), dtype=torch.uint8, device=self.dev)
        self.pr, self.res = pr, res

    def run(self):
        st = self.lib.hhmm_draw_stats_gauss_device(C.byref(self.pr.req), C.byref(self.res), self.ws.data_ptr(),
                                                   self.ws.numel(), torch.cuda.current_stream().cuda_stream)
        if st < 0:
            raise RuntimeError(self.lib.hhmm_last_error().decode())
        torch.cuda.synchronize()
        return st

    def stats(self):
        out = {name: v.cpu().numpy().reshape(self.shapes[name], order="F") for name, v in self.out.items()}
        out["pair_status"] = self.status.cpu().numpy()
        return out
