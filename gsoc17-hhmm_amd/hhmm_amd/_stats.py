"""What the "statistics per (series, draw) pair" entries share on the Python side.

hhmm_estep, hhmm_estep_large, hhmm_draw_stats, hhmm_draw_stats_gauss, hhmm_draw_stats_large and hhmm_expected_stats take
an hhmm_request and fill an hhmm_estep_result (include/hhmm_estep.h);
hhmm_estep_io fills its own hhmm_estep_io_result (`result_cls`).  They differ in the draw arrays they read, the statistics they return and whether
they consume uniforms.  `request()` builds the pair with the shape checks,
`add_uniforms()` attaches the uniforms of a draw, `call()` runs a host entry,
and `DeviceStats` keeps a prepared request on the GPU for repeated calls of a
device entry (the Gibbs samplers, the tests' device-path helpers).
"""
import ctypes as C

import numpy as np

from . import _abi
from .api import HHMMError, PreparedRequest, _f64


def request(model, data, draws, pairing, device, param_shapes, stat_shapes, result_cls=_abi.EstepResult):
    """(PreparedRequest, result_cls(), {name: array}) with the shape checks.

    param_shapes(S, K, L) and stat_shapes(P, K, L) return {name: shape} of the
    draw arrays the entry reads and of the statistics it returns."""
    pr = PreparedRequest(model, data, draws, [], pairing, device)
    if pairing == "zip" and pr.N != pr.S:
        raise ValueError(f"zip pairing needs n_series ({pr.N}) == n_draws ({pr.S})")
    L = int(data.get("L", 0))
    for name, shape in param_shapes(pr.S, pr.K, L).items():
        if name not in draws:
            raise ValueError(f"{model} needs the draw array {name}")
        if np.shape(draws[name]) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {np.shape(draws[name])}")
    res = result_cls()
    out = {}
    for name, shape in stat_shapes(pr.P, pr.K, L).items():
        out[name] = np.full(shape, np.nan, dtype=np.float64, order="F")
        setattr(res, name, out[name].ctypes.data)
    res.pair_status = pr.status.ctypes.data
    return pr, res, out


def add_uniforms(pr, uniforms):
    """Points pr.req.ffbs_u at the uniforms of the draw, shape (P, T_max)."""
    if uniforms is None:
        raise ValueError("the draw needs uniforms of shape (P, T_max)")
    uu = _f64(uniforms)
    if uu.shape != (pr.P, pr.Tmax):
        raise ValueError(f"uniforms must have shape {(pr.P, pr.Tmax)}, got {uu.shape}")
    pr.req.ffbs_u = pr._ptr(uu)


def call(lib, entry, pr, res, out, return_status):
    """Runs the host entry hhmm_<entry> on a prepared request; returns `out`."""
    st = getattr(lib, "hhmm_" + entry)(C.byref(pr.req), C.byref(res))
    if st < 0:
        raise HHMMError(st, lib.hhmm_last_error().decode())
    if return_status:
        out["pair_status"] = pr.status
        out["status"] = st
    return out


class DeviceStats:
    """A prepared request on torch's current GPU, for hhmm_<entry>_device.

    The arrays the request points at (pr.keep: data, draws, uniforms if any)
    move to the device once and the request is re-pointed at them; `arrays`
    has the draw arrays by name, so a caller can update them in place.  The
    statistics (`out`: flat tensors in the ABI's first-index-fastest layout,
    NaN until a run), the pair status (-1 until a run) and the workspace live
    there too.  run() enqueues the entry on torch's current stream."""

    def __init__(self, lib, entry, pr, res, shapes):
        import torch
        self._torch = torch
        self.lib, self.pr, self.res, self.shapes = lib, pr, res, dict(shapes)
        self._entry = getattr(lib, f"hhmm_{entry}_device")
        dev = self.dev = torch.device("cuda", torch.cuda.current_device())
        keep = {arr.ctypes.data: torch.from_numpy(np.asarray(arr).reshape(-1, order="F").copy()).to(dev)
                for arr in pr.keep}
        self.arrays = {}
        for struct, named in ((pr.req.data, {}), (pr.req.draws, self.arrays)):
            for name, ctype in struct._fields_:
                v = getattr(struct, name)
                if ctype is C.c_void_p and v and v in keep:
                    setattr(struct, name, keep[v].data_ptr())
                    named[name] = keep[v]
        if pr.req.ffbs_u in keep:
            pr.req.ffbs_u = keep[pr.req.ffbs_u].data_ptr()
        self._keep = keep
        self.out = {}
        for name, shape in self.shapes.items():
            self.out[name] = torch.full((int(np.prod(shape)),), float("nan"), dtype=torch.float64, device=dev)
            setattr(res, name, self.out[name].data_ptr())
        self.status = torch.full((pr.P,), -1, dtype=torch.int32, device=dev)
        res.pair_status = self.status.data_ptr()
        wsb = C.c_size_t(0)
        if getattr(lib, f"hhmm_{entry}_workspace_size")(C.byref(pr.req), C.byref(wsb)) < 0:
            raise HHMMError(_abi.ERR_INVALID_ARGUMENT, lib.hhmm_last_error().decode())
        self.ws = torch.empty(max(int(wsb.value), 256), dtype=torch.uint8, device=dev)

    def run(self):
        st = self._entry(C.byref(self.pr.req), C.byref(self.res), self.ws.data_ptr(), self.ws.numel(),
                         self._torch.cuda.current_stream().cuda_stream)
        if st < 0:
            raise HHMMError(st, self.lib.hhmm_last_error().decode())
        return st

    def stats(self):
        """The statistics and pair_status on the host, in the host entries' layout."""
        out = {name: v.cpu().numpy().reshape(self.shapes[name], order="F") for name, v in self.out.items()}
        out["pair_status"] = self.status.cpu().numpy()
        return out
