"""mfhip -- MI355X-native DSGD / online matrix factorisation (host mirror of the reference API).

The compute path is libmfhip.so (hand-written HIP for gfx950 behind a C ABI, include/mfhip.h);
this package is the Python equivalent of the Scala entry points that bind it.
"""
from . import _lib, jvm, negsample, synth
from ._lib import SEEN, MFError, MFNoDeviceError, device_count, version
from .als import ALS, MatrixFactorizationModel, StreamingALS
from .context import Context, Prequential, RankMetrics, block_update
from .core import (FactorInitializer, FactorInitializerDescriptor, Factors, FactorUpdater, FactorVector,
                   ItemUpdate, MockFactorUpdater, PseudoRandomFactorInitializer,
                   PseudoRandomFactorInitializerDescriptor, RandomFactorInitializer,
                   RandomFactorInitializerDescriptor, Rating, SGDUpdater, UserUpdate)
from .dsgd import DSGDforMF, LearningRateMethod
from .online import OnlineMF
from .prequential import PrequentialEvaluator, host_prequential
from .ranking import RankingMetrics
from .ratings_io import read_ratings

__all__ = [
    "MFError", "MFNoDeviceError", "device_count", "version", "Context", "block_update", "DSGDforMF",
    "LearningRateMethod", "OnlineMF", "Rating", "FactorVector", "Factors", "FactorUpdater", "SGDUpdater",
    "MockFactorUpdater", "FactorInitializer", "FactorInitializerDescriptor", "PseudoRandomFactorInitializer",
    "PseudoRandomFactorInitializerDescriptor", "RandomFactorInitializer", "RandomFactorInitializerDescriptor",
    "UserUpdate", "ItemUpdate", "read_ratings", "ALS", "MatrixFactorizationModel", "StreamingALS",
    "RankMetrics", "RankingMetrics", "Prequential", "PrequentialEvaluator", "host_prequential",
    "SEEN",
]
