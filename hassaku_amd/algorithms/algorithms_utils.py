"""Name -> class registry (algorithms/algorithms_utils.py:12-30).  Filled: the slot on the hot path (mf), its
bias-only sibling (sgdbias), the anchor / prototype models that share the embedding gather and the
neighbourhood models (uknn, iknn), the linear model (ease), the graph model (p3alpha) and the truncated SVD (svd); the
reference's other algorithms are out of scope, except its neural model (dmf), which trains
like the other SGD models but on a sparse first layer.

The registry has seven families.  `AlgorithmsEnum` holds the SGD-trained models: iterating it lists those six, as it
always has.  `SparseAlgorithmsEnum` holds the neighbourhood models, `LinearAlgorithmsEnum` the linear one and
`GraphAlgorithmsEnum` the random-walk one and `FactorAlgorithmsEnum` the one-shot factorisation (all fitted once on
the train CSR).  Every family is reachable by name through `AlgorithmsEnum` (`AlgorithmsEnum['iknn']`,
`AlgorithmsEnum.ease`, `AlgorithmsEnum.p3alpha`, `AlgorithmsEnum.svd`), so every caller
that resolves a slot by name -- run_experiment.py, the experiment helpers -- takes any of them.  `ALGORITHM_NAMES` lists the first two families, `ALL_ALGORITHM_NAMES` the first three and
`REGISTERED_ALGORITHM_NAMES` the first four and `CLI_ALGORITHM_NAMES` the first five (the earlier tuples keep their
contents).  `NeuralAlgorithmsEnum` holds `dmf`, trained by the Trainer like the first family;
`EXPERIMENT_ALGORITHM_NAMES` = `CLI_ALGORITHM_NAMES` + ('dmf',).  `TagAlgorithmsEnum` holds `ecf`, trained by the
Trainer too, on a dataset that carries the item x tag matrix; `RUNNABLE_ALGORITHM_NAMES` =
`EXPERIMENT_ALGORITHM_NAMES` + ('ecf',).  Callers use only a slot's `.name` and `.value`.

`WeightedFactorAlgorithmsEnum` holds `als` (implicit-feedback alternating least squares, fitted on the train CSR like
the other closed-form models).  It is not among the families `AlgorithmsEnum` looks through: `AlgorithmsEnum['als']`
raises KeyError as it always has, and `RUNNABLE_ALGORITHM_NAMES` keeps its contents.  `algorithm_by_name(name)`
resolves every slot, the new family included, and `OFFERED_ALGORITHM_NAMES` = `RUNNABLE_ALGORITHM_NAMES` + ('als',)
lists them.

`SparseLinearAlgorithmsEnum` holds `slim` (SLIM, one non-negative elastic net per item, fitted on the train CSR) in the
same way: not among the families `AlgorithmsEnum` looks through (`AlgorithmsEnum['slim']` raises KeyError),
resolved by `algorithm_by_name('slim')`, and `OFFERED_ALGORITHM_NAMES` keeps its contents.
`AVAILABLE_ALGORITHM_NAMES` = `OFFERED_ALGORITHM_NAMES` + ('slim',) is what run_experiment.py offers.
"""
from enum import Enum, EnumMeta

from hassaku_amd.algorithms.ecf_alg import ECF
from hassaku_amd.algorithms.graph_algs import P3alpha
from hassaku_amd.algorithms.knn_algs import ItemKNN, UserKNN
from hassaku_amd.algorithms.linear_algs import EASE, SLIM
from hassaku_amd.algorithms.mf_algs import AlternatingLeastSquare, SVDAlgorithm
from hassaku_amd.algorithms.neural_algs import DeepMatrixFactorization
from hassaku_amd.algorithms.proto_alg import ACF, IProtoMF, UIProtoMF, UProtoMF
from hassaku_amd.algorithms.sgd_alg import SGDBaseline, SGDMatrixFactorization


class SparseAlgorithmsEnum(Enum):
    uknn = UserKNN
    iknn = ItemKNN


class LinearAlgorithmsEnum(Enum):
    ease = EASE


class GraphAlgorithmsEnum(Enum):
    p3alpha = P3alpha


class FactorAlgorithmsEnum(Enum):
    svd = SVDAlgorithm


class NeuralAlgorithmsEnum(Enum):
    dmf = DeepMatrixFactorization


class TagAlgorithmsEnum(Enum):
    ecf = ECF


class WeightedFactorAlgorithmsEnum(Enum):   # reached through algorithm_by_name(), not through AlgorithmsEnum
    als = AlternatingLeastSquare


class SparseLinearAlgorithmsEnum(Enum):    # likewise
    slim = SLIM


_OTHER_FAMILIES = (SparseAlgorithmsEnum, LinearAlgorithmsEnum, GraphAlgorithmsEnum, FactorAlgorithmsEnum,
                   NeuralAlgorithmsEnum, TagAlgorithmsEnum)


class _RegistryMeta(EnumMeta):
    """Looks a name up among the SGD slots first, then among the sparse-matrix, the linear, the graph, the factor, the
    neural and the tag slots."""

    def __getitem__(cls, name):
        if name in cls._member_map_:
            return cls._member_map_[name]
        for family in _OTHER_FAMILIES:
            if name in family.__members__:
                return family[name]
        raise KeyError(name)

    def __getattr__(cls, name):
        if not name.startswith('_'):
            for family in _OTHER_FAMILIES:
                if name in family.__members__:
                    return family[name]
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
ALL_ALGORITHM_NAMES = ALGORITHM_NAMES + tuple(m.name for m in LinearAlgorithmsEnum)
REGISTERED_ALGORITHM_NAMES = ALL_ALGORITHM_NAMES + tuple(m.name for m in GraphAlgorithmsEnum)
CLI_ALGORITHM_NAMES = REGISTERED_ALGORITHM_NAMES + tuple(m.name for m in FactorAlgorithmsEnum)
EXPERIMENT_ALGORITHM_NAMES = CLI_ALGORITHM_NAMES + tuple(m.name for m in NeuralAlgorithmsEnum)
RUNNABLE_ALGORITHM_NAMES = EXPERIMENT_ALGORITHM_NAMES + tuple(m.name for m in TagAlgorithmsEnum)
OFFERED_ALGORITHM_NAMES = RUNNABLE_ALGORITHM_NAMES + tuple(m.name for m in WeightedFactorAlgorithmsEnum)
AVAILABLE_ALGORITHM_NAMES = OFFERED_ALGORITHM_NAMES + tuple(m.name for m in SparseLinearAlgorithmsEnum)


def algorithm_by_name(name: str):
    """The slot called `name`: `AlgorithmsEnum[name]`, or the member of `WeightedFactorAlgorithmsEnum` or of
    `SparseLinearAlgorithmsEnum`."""
    try:
        return AlgorithmsEnum[name]
    except KeyError:
        pass
    if name in SparseLinearAlgorithmsEnum.__members__:
        return SparseLinearAlgorithmsEnum[name]
    return WeightedFactorAlgorithmsEnum[name]
