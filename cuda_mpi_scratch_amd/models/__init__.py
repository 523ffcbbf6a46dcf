"""Workloads ("model families") of the suite: 2D stencil, ping-pong, dot product."""
from .cg2d import CgConfig, ConjugateGradient2D  # noqa: F401
from .dot import DotProduct  # noqa: F401
from .heat2d import HeatConfig, ImplicitHeat2D  # noqa: F401
from .multigrid2d import Multigrid2D, MultigridConfig  # noqa: F401
from .pcg2d import MultigridPcg2D, PcgConfig  # noqa: F401
from .pingpong import PingPong, parse_sweep, reference_report  # noqa: F401
from .stencil2d import Stencil2D, StencilConfig, format_tile  # noqa: F401
