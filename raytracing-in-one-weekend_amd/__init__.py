"""MI355X-native sample-batch path for renaudbedard/raytracing-in-one-weekend.

Package layout:
  abi.py     ctypes mirror of include/rtow.h
  lib.py     loader for csrc/librtow_hip.so (the C-ABI product library; fails loudly if missing)
  host.py    host-side mirror of the reference's job structs (SampleBatchJob, CombineJob, DenoiseJob, ShadeHitsJob, ...)
  scenes.py  synthetic benchmark scenes (input preparation, shared by product and tests)
  csrc/      hand-written HIP (gfx950) kernels + the C ABI implementation

The directory name contains '-' so it is loaded with importlib (see tests/conftest.py, bench.py):
    rtow = importlib.import_module("raytracing-in-one-weekend_amd")
"""
from . import abi, host, lib, scenes  # noqa: F401
from .host import (BloomJob, CombineJob, Context, DenoiseJob, DenoiseVarianceJob, DeviceBuffer, EstimateMomentsJob, ExposureJob, FinalizeTexturesJob, MomentsJob, NoiseMaskJob, PixelListJob, RectifyHistoryJob, ReduceMetricsJob, ReprojectBilinearJob, ReprojectJob, ReprojectMomentsJob, SampleBatchJob, ShadeHitsJob, ToneMapJob, UpsampleJob,  # noqa: F401
                   sample_batch_chain_adaptive_device, sample_batch_chain_device, sample_batch_chain_host, sample_batch_group_device, sample_batch_host, sample_pixels_device, build_pixel_list, refine_noisy_pixels)

__all__ = ["abi", "host", "lib", "scenes", "Context", "DeviceBuffer", "SampleBatchJob", "CombineJob", "DenoiseJob", "FinalizeTexturesJob",
           "ReduceMetricsJob", "ReprojectJob", "ShadeHitsJob", "UpsampleJob", "sample_batch_host", "sample_batch_chain_device", "sample_batch_chain_adaptive_device", "sample_batch_chain_host", "sample_batch_group_device",
           "PixelListJob", "build_pixel_list", "sample_pixels_device", "MomentsJob", "DenoiseVarianceJob", "ReprojectMomentsJob", "EstimateMomentsJob", "NoiseMaskJob", "refine_noisy_pixels", "RectifyHistoryJob", "ReprojectBilinearJob", "ExposureJob", "ToneMapJob", "BloomJob"]
