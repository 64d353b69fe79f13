"""``fv3fit``-shaped model API for the column MLP: Predictor ABC, the name-file io registry,
the dataset <-> array adapter, and the HIP dense predictor (registered as ``"hip-dense"``; its sibling with the
column water budget closed is ``"hip-precipitative"``)."""
from . import io
from .io import dump, load
from .predictor import Predictor
from .stacking import SAMPLE_DIM_NAME, match_prediction_to_input_coords, stack
from .dense import DenseHyperparameters, HipDenseModel, spec_from_arrays, train_dense_model
from .input_sensitivity import InputSensitivity, JacobianInputSensitivity, RandomForestInputSensitivity
from .testing import ConstantOutputNoveltyDetector, ConstantOutputPredictor
from .derived import DerivedMapping, DerivedModel
from .models import (CombinedOutputModel, EnsembleModel, SquashedOutputConfig, SquashedOutputModel, TaperConfig, TaperedModel,
                     vertical_tapering_scale_factors)
from .data_transform import DATA_TRANSFORM_REGISTRY, ChainedDataTransform, DataTransform
from .novelty import (MinMaxNoveltyDetector, NoveltyDetector, OCSVMNoveltyDetector, get_taper_function, taper_decay, taper_mask,
                      taper_ramp)
from .transformed import OutOfSampleModel, TransformedPredictor
from .forest import RandomForest, RandomForestHyperparameters, train_random_forest
from .conv import ConvolutionalHyperparameters, HipConvolutionalModel, conv_spec_from_arrays, train_convolutional_model
from .precipitative import (HipPrecipitativeModel, PrecipitativeHyperparameters, precipitative_spec_from_arrays,
                            train_precipitative_model)
from .emulator_train import (ArchitectureConfig, CustomLoss, MicrophysicsConfig, NormFactory, OptimizerConfig, SliceConfig,
                             TransformedParameters, TransformedTrainingResult, train_transformed_model)
from .graph import (GraphHyperparameters, GraphUNetTwin, HipGraphAutoregressor, graph_unet_spec_from_state_dict,
                    state_dict_from_spec, train_graph_model, twin_from_spec)
from .cyclegan import (GeneratorTwin, HipCycleGAN, cyclegan_spec_from_state_dict, cyclegan_state_dict_from_spec,
                       generator_spec_from_state_dict)
from .cyclegan_train import (CycleGANGeneratorConfig, CycleGANHyperparameters, CycleGANNetworkConfig, CycleGANOptimizerConfig,
                             CycleGANSchedulerConfig, CycleGANTrainer, CycleGANTrainingConfig, DiscriminatorConfig, DiscriminatorTwin,
                             HipDiscriminator, ImagePool, LossConfig, train_cyclegan)
from .fmr import (HipFullModelReplacement, RecurrentGeneratorTwin, fmr_spec_from_state_dict, fmr_state_dict_from_spec,
                  recurrent_generator_spec_from_state_dict, recurrent_twin_from_spec)
from .fmr_train import (FMRHyperparameters, FMRNetworkConfig, FMRTrainer, FMRTrainingConfig, RecurrentDiscriminatorConfig,
                        RecurrentGeneratorConfig, train_fmr)
from .reservoir import (BatchLinearRegressor, BatchLinearRegressorHyperparameters, CubedsphereSubdomainConfig, DenseAutoencoder,
                        DenseAutoencoderHyperparameters, HybridReservoirComputingModel, HybridReservoirDatasetAdapter,
                        NotFittedError, Reservoir, ReservoirComputingModel, ReservoirDatasetAdapter, ReservoirHyperparameters,
                        ReservoirTrainingConfig, SkTransformer, SynchronizationTracker, TransformerGroup,
                        split_multi_subdomain_model, train_dense_autoencoder, train_reservoir_model)

__all__ = [
    "ChainedDataTransform", "ConstantOutputNoveltyDetector", "DATA_TRANSFORM_REGISTRY", "DataTransform", "MinMaxNoveltyDetector", "NoveltyDetector", "OCSVMNoveltyDetector",
    "OutOfSampleModel", "RandomForest", "HipConvolutionalModel", "conv_spec_from_arrays", "HybridReservoirComputingModel", "HybridReservoirDatasetAdapter",
    "ReservoirComputingModel", "ReservoirDatasetAdapter", "split_multi_subdomain_model", "TransformedPredictor", "get_taper_function", "taper_decay", "taper_mask", "taper_ramp",
    "CombinedOutputModel", "ConstantOutputPredictor", "DenseHyperparameters", "DerivedMapping", "DerivedModel", "EnsembleModel", "SquashedOutputConfig",
    "SquashedOutputModel", "TaperConfig", "TaperedModel", "vertical_tapering_scale_factors", "HipDenseModel", "Predictor", "SAMPLE_DIM_NAME", "dump", "io",
    "load", "match_prediction_to_input_coords", "spec_from_arrays", "stack", "train_dense_model",
    "HipPrecipitativeModel", "PrecipitativeHyperparameters", "precipitative_spec_from_arrays", "train_precipitative_model",
    "GraphHyperparameters", "GraphUNetTwin", "HipGraphAutoregressor", "graph_unet_spec_from_state_dict", "state_dict_from_spec",
    "train_graph_model", "twin_from_spec",
    "GeneratorTwin", "HipCycleGAN", "cyclegan_spec_from_state_dict", "cyclegan_state_dict_from_spec", "generator_spec_from_state_dict",
    "CycleGANGeneratorConfig", "CycleGANHyperparameters", "CycleGANNetworkConfig", "CycleGANOptimizerConfig", "CycleGANSchedulerConfig",
    "CycleGANTrainer", "CycleGANTrainingConfig", "DiscriminatorConfig", "DiscriminatorTwin", "HipDiscriminator", "ImagePool", "LossConfig", "train_cyclegan",
    "HipFullModelReplacement", "RecurrentGeneratorTwin", "fmr_spec_from_state_dict", "fmr_state_dict_from_spec",
    "recurrent_generator_spec_from_state_dict", "recurrent_twin_from_spec",
    "FMRHyperparameters", "FMRNetworkConfig", "FMRTrainer", "FMRTrainingConfig", "RecurrentDiscriminatorConfig", "RecurrentGeneratorConfig",
    "train_fmr",
    "DenseAutoencoder", "DenseAutoencoderHyperparameters", "SkTransformer", "train_dense_autoencoder",
    "BatchLinearRegressor", "BatchLinearRegressorHyperparameters", "CubedsphereSubdomainConfig", "NotFittedError", "Reservoir",
    "ReservoirHyperparameters", "ReservoirTrainingConfig", "SynchronizationTracker", "TransformerGroup", "train_reservoir_model",
    "InputSensitivity", "JacobianInputSensitivity", "RandomForestInputSensitivity",
    "RandomForestHyperparameters", "train_random_forest",
    "ConvolutionalHyperparameters", "train_convolutional_model",
    "ArchitectureConfig", "CustomLoss", "MicrophysicsConfig", "NormFactory", "OptimizerConfig", "SliceConfig", "TransformedParameters",
    "TransformedTrainingResult", "train_transformed_model",
]
