from .aggregators import (
    BulyanAggregator,
    CyclicAggregator,
    GeoMedianAggregator,
    KrumAggregator,
    MeanAggregator,
    MeanAroundAggregator,
    MultiKrumAggregator,
    TrimmedMeanAggregator,
    VoteAggregator,
)
from .comm import Communicator
from .flat import FlatSpace
from .trainer import Trainer

__all__ = [
    "Communicator",
    "FlatSpace",
    "Trainer",
    "MeanAggregator",
    "VoteAggregator",
    "GeoMedianAggregator",
    "KrumAggregator",
    "MultiKrumAggregator",
    "BulyanAggregator",
    "TrimmedMeanAggregator",
    "MeanAroundAggregator",
    "CyclicAggregator",
]
