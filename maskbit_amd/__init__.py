"""maskbit_amd: MI355X-native MaskBit sampling engine (hand-written gfx950 HIP kernels behind the
reference's LFQBert / ConvVQModel / sample() call surface)."""
from .base_model import BaseModel
from .bert import Bert, LFQBert
from .conv_vqgan import ConvVQModel
from .taming_vqgan import OriginalVQModel
from .factorization import combine_factorized_tokens, split_factorized_tokens
from .masking import get_masking_ratio
from .sampling import SampleRequest, sample, sample_requests, sample_seeded
from .session import Finished, SamplingSession
from .evaluator import TokenizerEvaluator
from .generator_evaluator import GeneratorEvaluator, frechet_distance, get_covariance, inception_score
from .manifold import knn_radii, manifold_coverage, precision_recall
from .lpips import LPIPS
from .perceptual import PerceptualLoss, create_perception_loss
from .discriminator import NLayerDiscriminatorv2, VQGANLoss, create_discriminator
from .image_transform import ImageTransform, transformed
from .inception import InceptionV3, get_inception_model
from .editing import inpaint, sample_from_tokens
from .checkpoint_check import CheckpointReport, check_checkpoint
from .validation import MLMLoss, MaskedTokenEvaluator, get_mask_tokens
from .harness import (eval_generation, eval_labels, eval_masked_prediction, eval_reconstruction, generate_uint8, mask_token_for,
                      to_evaluator_uint8)

__all__ = ["BaseModel", "Bert", "LFQBert", "ConvVQModel", "OriginalVQModel", "sample", "sample_seeded", "SampleRequest", "sample_requests", "SamplingSession", "Finished", "get_masking_ratio",
           "combine_factorized_tokens", "split_factorized_tokens", "eval_labels", "generate_uint8", "mask_token_for", "to_evaluator_uint8",
           "TokenizerEvaluator", "eval_reconstruction", "inpaint", "sample_from_tokens",
           "get_mask_tokens", "MLMLoss", "MaskedTokenEvaluator", "eval_masked_prediction", "LPIPS", "PerceptualLoss", "create_perception_loss",
           "NLayerDiscriminatorv2", "VQGANLoss", "create_discriminator",
           "GeneratorEvaluator", "eval_generation", "frechet_distance", "inception_score", "get_covariance",
           "InceptionV3", "get_inception_model", "check_checkpoint", "CheckpointReport",
           "knn_radii", "manifold_coverage", "precision_recall", "ImageTransform", "transformed"]
