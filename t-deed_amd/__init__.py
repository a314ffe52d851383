"""tdeed_amd -- MI355X-native (gfx950) T-DEED hot path.

Directory name is ``t-deed_amd`` (build contract); import name is ``tdeed_amd``
(see the shim ``tdeed_amd.py`` at the repo root).

Importing the package does not touch the GPU.  Every compute entry point goes
through the C-ABI library ``csrc/libtdeed_hip.so`` (see ``include/tdeed_hip.h``);
there is no CPU or eager-PyTorch fallback: a missing library raises
``tdeed_amd._lib.HipLibraryMissing`` at the first op.
"""
# Importing the package changes no runtime or device setting: the number of hardware queues (GPU_MAX_HW_QUEUES) is the HIP
# runtime's default.  More queues were measured to help only the host-fed rate (1730 -> 2140 clips/s at cfg2 with 8;
# device-resident throughput unchanged), not enough to make a process claim more than its share of a shared GPU.

__version__ = "0.1.0"
