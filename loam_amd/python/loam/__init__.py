"""`import loam` — the Python surface of the reference (python/loam_bindings.cpp) on the MI355X back end."""
from .loam_python import *  # noqa: F401,F403
from .loam_python import (FeatureExtractionParams, LidarParams, LoamFeatures, Pose3d, Quaterniond,  # noqa: F401
                          RegistrationDetail, RegistrationIterationInfo, RegistrationParams,
                          RegistrationTerminationType, computeCurvature, computeValidPoints, extractFeatures,
                          registerFeatures)
from .loam_python import deskewScan, registerScanSequence  # noqa: F401  (extensions: scan sequences)
from .loam_python import RegistrationInformation, registrationInformation  # noqa: F401  (extension: information matrix)
from .loam_python import PoseGraph, PoseGraphParams, PoseGraphSummary  # noqa: F401  (extension: pose graph)
from .loam_python import CloudMap, CloudMapParams  # noqa: F401  (extension: cloud map)
from .loam_python import VisibilityParams, removeDynamicPoints, visibilityVotes  # noqa: F401  (extension: map cleaning)
from .loam_python import LocalizeParams, LocalizeResult, SurfelMap, SurfelMapParams  # noqa: F401  (extension: surfel map and localisation)
