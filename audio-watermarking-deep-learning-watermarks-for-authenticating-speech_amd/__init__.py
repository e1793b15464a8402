"""MI355X-native watermark embed + detect hot path (drop-in for py/main16.py's Generator / Detector /
delta post-processing / loss stack).  Import name: ``awm_amd`` (see awm_amd.py at the repo root)."""
from .modules import Detector, Generator, ResBlock, load_state_dict_strip_prefix
from .losses import (MultiScaleMelLoss, TFLoudnessLoss, clamp_peak, detection_losses, detection_losses_masked, fir_lowpass, high_freq_penalty,
                     l1_to_zero, limit_rms, postprocess)
from .step import LOSS_WEIGHTS, forward_losses, train_step, eval_forward
from .optim import FlatAdam
from .codec import PcmCodec, encode_pcm16, perceptual_postprocess
from .attacks import (Convolved, Distortion, Lowpass, LpcCodec, NoiseSuppress, PitchShift, Resampled, Reverb, Splice, TimeStretch, TimeWarp, TransformCodec, echo_ir,
                      evaluate_localization, evaluate_robustness, evaluate_robustness_by_class, pack_labels, row_splice_spans, splice_rows_host, unpack_labels)
from . import attacks, draws
from .inference import (compute_si_snr, detect_prob, detect_watermark, detect_waveform, embed_waveform, evaluate_batches,
                        evaluate_unseen_file, generate_watermarked_audio, load_audio, locate_watermark, lowpass_biquad, pcm16, read_audio, resample, resample_add, Resample,
                        save_audio,
                        save_audio_float)
from .quality import stoi, nmr
from .masking import masking, MaskingLoss
from .suppress import noise_suppress
from . import quality
from .detection import (auc, calibrate_threshold, detection_report, eer, evaluate_detection, operating_point, roc_curve, tpr_at_fpr)
from . import detection
from .curate import (butter_bandpass_sos, classify_speech_noise, clip_features, curate_files, dct_ortho, is_silent, prepare_recording, slaney_mel)
from . import curate
from . import dsp, ops
from . import checkpoint
from . import main14b_2
from . import distributed
from ._lib import lib, LIB_PATH

__all__ = ["Generator", "Detector", "ResBlock", "load_state_dict_strip_prefix", "MultiScaleMelLoss", "TFLoudnessLoss",
           "fir_lowpass", "clamp_peak", "limit_rms", "postprocess", "high_freq_penalty", "detection_losses", "l1_to_zero",
           "forward_losses", "train_step", "eval_forward", "LOSS_WEIGHTS", "FlatAdam", "distributed", "checkpoint", "main14b_2", "generate_watermarked_audio", "detect_watermark", "embed_waveform",
           "detect_waveform", "detect_prob", "evaluate_unseen_file", "evaluate_batches", "compute_si_snr", "load_audio", "save_audio", "save_audio_float", "lowpass_biquad", "pcm16", "resample", "Resample", "resample_add", "read_audio", "perceptual_postprocess", "PcmCodec", "encode_pcm16",
           "attacks", "draws", "Distortion", "Lowpass", "Resampled", "TransformCodec", "LpcCodec", "Convolved", "Reverb", "TimeWarp", "TimeStretch", "PitchShift", "echo_ir", "evaluate_robustness", "evaluate_robustness_by_class",
           "Splice", "evaluate_localization", "row_splice_spans", "splice_rows_host", "pack_labels", "unpack_labels", "detection_losses_masked",
           "locate_watermark",
           "stoi", "quality",
           "detection", "evaluate_detection", "detection_report", "roc_curve", "auc", "eer", "tpr_at_fpr", "calibrate_threshold", "operating_point",
           "curate", "clip_features", "classify_speech_noise", "is_silent", "prepare_recording", "curate_files", "butter_bandpass_sos", "slaney_mel", "dct_ortho",
           "lib", "LIB_PATH",
           "NoiseSuppress", "noise_suppress",
           "masking", "MaskingLoss", "nmr"]
