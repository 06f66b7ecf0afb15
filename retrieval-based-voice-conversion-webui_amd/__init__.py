"""MI355X-native hot path of RVC inference (imported as ``rvc_amd``).

faiss IVF-Flat retrieval + NSF-HiFi-GAN generator as hand-written HIP for gfx950 behind the
reference's own Python call surface.  See DESIGN.md / INTEGRATION.md.
"""
from . import _lib
from ._lib import RvcmiError, build
from .ivf import IVFFlatHIP, extract_index_ivf, index_factory, kmeans, read_index, reduce_features, train_index, write_index
from .front import FrontHIP, front_config_from_reference, infer_hip
from .nsf import GeneratorHIP, NSFGeneratorHIP, config_from_reference
from .pipeline import retrieve_blend
from . import glue
from .glue import cut_count, cut_points, filtfilt, highpass16k
from .gru import GRUHIP, accelerate_rmvpe
from .unet import UNetHIP, accelerate_rmvpe_unet, restore_rmvpe_unet
from .rmvpe import RMVPEHIP
from .hubert import (HubertEncoderHIP, HubertFrontHIP, HubertLayerHIP, accelerate_hubert, accelerate_hubert_layers, hubert_enc_on,
                     restore_hubert_layers, supported_layer, batch_capable, extract_features_batch, frame_mask, hubert_batch_on, hubert_on, plan_groups,
                     restore_hubert, sample_mask)
from .synthesizer import accelerate_synthesizer, get_synthesizer, load_synthesizer
from . import dist
from .install import install, uninstall
from .gate import TorchGateBank, TorchGateHIP
from .realtime import PitchCache, RealtimeBank, RealtimeStream, RealtimeVC, RealtimeVCBatch, SessionSliders, SincResample, SincResampleRagged, f0_extractor_frame, formant_geometry, sinc_resample_kernel, stream_geometry

__all__ = [
    "RvcmiError", "build", "IVFFlatHIP", "read_index", "write_index", "train_index", "reduce_features", "kmeans", "index_factory", "extract_index_ivf", "GeneratorHIP", "NSFGeneratorHIP",
    "config_from_reference", "FrontHIP", "front_config_from_reference", "infer_hip", "retrieve_blend", "accelerate_synthesizer", "get_synthesizer", "load_synthesizer", "dist", "glue", "install", "uninstall", "RealtimeVC", "PitchCache", "f0_extractor_frame", "SincResample", "SincResampleRagged", "formant_geometry", "sinc_resample_kernel", "GRUHIP", "accelerate_rmvpe",
    "UNetHIP", "accelerate_rmvpe_unet", "restore_rmvpe_unet", "RMVPEHIP", "HubertFrontHIP", "accelerate_hubert", "restore_hubert", "hubert_on", "hubert_batch_on", "batch_capable", "extract_features_batch",
    "frame_mask", "sample_mask", "plan_groups", "HubertEncoderHIP", "HubertLayerHIP", "accelerate_hubert_layers", "restore_hubert_layers", "supported_layer", "hubert_enc_on",
    "RealtimeStream", "RealtimeBank", "RealtimeVCBatch", "SessionSliders", "stream_geometry", "TorchGateHIP", "TorchGateBank", "cut_points", "cut_count", "filtfilt", "highpass16k",
]
