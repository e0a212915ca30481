"""Name -> class registry (algorithms/algorithms_utils.py:12-30).  Filled: the slot on the hot path (mf), its
bias-only sibling (sgdbias), the anchor / prototype models that share the embedding gather and the
neighbourhood models (uknn, iknn); the reference's other ten algorithms are out of scope.

The registry has two families.  `AlgorithmsEnum` holds the SGD-trained models: iterating it lists those six, as it
always has.  `SparseAlgorithmsEnum` holds the sparse-matrix models (fitted once on the train CSR).  Both families are
reachable by name through `AlgorithmsEnum` (`AlgorithmsEnum['iknn']`, `AlgorithmsEnum.uknn`), so every caller that
resolves a slot by name -- run_experiment.py, the experiment helpers -- takes either.  `ALGORITHM_NAMES` lists them all.
Callers use only a slot's `.name` and `.value`.
"""
from enum import Enum, EnumMeta

from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
from hassaku_amd.algorithms.proto_alg import ACF, IProtoMF, UIProtoMF, UProtoMF
from hassaku_amd.algorithms.sgd_alg import SGDBaseline, SGDMatrixFactorization


class SparseAlgorithmsEnum(Enum):
    uknn = UserKNN
    iknn = ItemKNN


class _RegistryMeta(EnumMeta):
    """Looks a name up among the SGD slots first, then among the sparse-matrix slots."""

    def __getitem__(cls, name):
        if name in cls._member_map_:
            return cls._member_map_[name]
        if name in SparseAlgorithmsEnum.__members__:
            return SparseAlgorithmsEnum[name]
        raise KeyError(name)

    def __getattr__(cls, name):
        if not name.startswith('_') and name in SparseAlgorithmsEnum.__members__:
            return SparseAlgorithmsEnum[name]
        if hasattr(EnumMeta, '__getattr__'):   # Python < 3.12 resolves members here
            return super().__getattr__(name)
        raise AttributeError(name)


class AlgorithmsEnum(Enum, metaclass=_RegistryMeta):
    mf = SGDMatrixFactorization
    sgdbias = SGDBaseline
    uprotomf = UProtoMF
    iprotomf = IProtoMF
    uiprotomf = UIProtoMF
    acf = ACF


ALGORITHM_NAMES = tuple(m.name for m in AlgorithmsEnum) + tuple(m.name for m in SparseAlgorithmsEnum)
