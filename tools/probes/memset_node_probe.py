"""Does a captured hipMemsetAsync replay as a node, in order, in front of the kernel node that follows it?  Only torch copy
kernels and runtime memsets on buffers of 1,024 bytes: every access is in bounds whatever the answer.
    python tools/probes/memset_node_probe.py        (recorded: profiles/r21/memset_node_probe.txt)"""
import ctypes
import os
import torch
hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hip.hipMemsetAsync.restype = ctypes.c_int
GUARD = 0x5ca7c4ed
raw = torch._C._cuda_getCurrentRawStream
res = []
for off, nbytes in [(0, 4), (0, 160), (80, 160), (208, 416)]:
    buf = torch.full((256,), GUARD, dtype=torch.int32, device="cuda")
    out = torch.full((256,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = hip.hipMemsetAsync(buf.data_ptr() + off, 0, nbytes, raw(torch.cuda.current_device()))
        out.copy_(buf)
    for r in range(3):
        buf.fill_(GUARD)
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        o = out.cpu()
        lo, hi = off // 4, (off + nbytes) // 4
        zeroed = bool((o[lo:hi] == 0).all())
        rest = bool((o[:lo] == GUARD).all() and (o[hi:] == GUARD).all())
        res.append(f"off={off} bytes={nbytes} rc={rc} replay={r} zeroed_in_front_of_the_copy={zeroed} rest_untouched={rest} "
                   f"head={o[lo:lo + 4].tolist()}")
print("\n".join(res))
