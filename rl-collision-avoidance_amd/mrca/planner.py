"""The global planner's Python side (include/mrca_env.h: mrca_planner_params, mrca_goal_fields, mrca_subgoals, and
mrca_los_params, mrca_subgoals_los: the per-tick call with line of sight).  The defaults are
the library's own (mrca_planner_default_params): they are stated once, in C."""
import dataclasses
import math

from . import _lib
from .params import ParamsMirror

INF = 0xFFFFFFFF                 # a field word: blocked, or no path
ON_GOAL, ON_PATH, NO_SLOT, NO_PATH = 1, 0, -1, -2
STATUS_NAMES = {ON_GOAL: "on_goal", ON_PATH: "on_path", NO_SLOT: "no_slot", NO_PATH: "no_path"}


@dataclasses.dataclass
class PlannerParams(ParamsMirror):
    """Mirror of mrca_planner_params; a field left ``None`` takes the library's default."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.PlannerParamsStruct, "mrca_planner_default_params", "--planner-param"
    stride: int = None                  # map cells per planning cell and axis, 1..8
    inflate: int = None                 # obstacles are grown by this many map cells, 0..64
    lookahead: int = None               # steps of the walk down the field, 1..256
    max_rounds: int = None              # at most this many relaxation launches; 0 = the library's derived bound

    @classmethod
    def for_grid(cls, grid, radius=0.35, lookahead_m=1.5, cell_m=0.1, max_rounds=0):
        """Metres -> cells on ``grid`` (a ``scenario.GridData``): planning cells of about ``cell_m``, obstacles grown by
        ``radius``, the subgoal about ``lookahead_m`` down the path."""
        stride = min(8, max(1, int(round(cell_m / grid.cell))))
        inflate = min(64, max(0, int(math.ceil(radius / grid.cell - 1e-6))))
        lookahead = min(256, max(1, int(round(lookahead_m / (grid.cell * stride)))))
        return cls(stride=stride, inflate=inflate, lookahead=lookahead, max_rounds=int(max_rounds))

    @classmethod
    def from_assignments(cls, items, base=None):
        """``["stride=1", "lookahead=20"]`` (the evaluator's --planner-param) on top of ``base`` -> PlannerParams."""
        return super().from_assignments(items, start=base and base.as_dict())


@dataclasses.dataclass
class LosParams(ParamsMirror):
    """Mirror of mrca_los_params; a field left ``None`` takes the library's default."""
    _STRUCT, _DEFAULTS, _FLAG = _lib.LosParamsStruct, "mrca_los_default_params", "--los-param"
    reach: int = None                   # steps of the path the line of sight may skip to, 1..256

    @classmethod
    def for_grid(cls, grid, reach_m=6.0, cell_m=0.1):
        """Metres -> cells on ``grid``: ``reach_m`` down the path in planning cells of about ``cell_m`` (the stride
        ``PlannerParams.for_grid`` picks for the same ``cell_m``)."""
        stride = min(8, max(1, int(round(cell_m / grid.cell))))
        return cls(reach=min(256, max(1, int(round(reach_m / (grid.cell * stride))))))

    @classmethod
    def from_assignments(cls, items, base=None):
        """``["reach=40"]`` (the evaluator's --los-param) on top of ``base`` -> LosParams."""
        return super().from_assignments(items, start=base and base.as_dict())


@dataclasses.dataclass
class GoalFields:
    """What ``VecStageWorld.plan_goals`` leaves: ``field`` int32[G,PH,PW] on the device (the u32 words of mrca_goal_fields seen
    through torch's int32: -1 is INF), the goal points float32[G,2] they belong to, ``slot`` int32[N] (which goal point each
    robot walks to; -1: none), the params they were planned with, and how many launches lowered something."""
    field: object
    goals: object
    slot: object
    params: PlannerParams
    rounds: int = 0

    @property
    def num_goals(self):
        return int(self.goals.shape[0])
