"""Device memory for the GPU tests, through torch and the HIP runtime the library shares with it (ntjoin_amd/capi.py): bytes up, bytes
at an address back.  No entry of the library is involved."""
import ctypes as C

import torch


def upload(text):
    "-> a uint8 tensor on the device holding the bytes (one spare byte, so that no text has a null address)"
    t = torch.zeros(len(text) + 1, dtype=torch.uint8, device="cuda")
    if text:
        t[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def download(address, n):
    "the n bytes of device memory at `address`"
    out = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if n:
        hip = C.CDLL(None)   # (the runtime is in the process already)
        assert hip.hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(address), C.c_size_t(n), 3) == 0   # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes()
