"""fsr_vln/memory/hmsg/graph/navigation_graph.py under its own import path (holoagent_amd/nav_graph.py)."""
from holoagent_amd.nav_graph import NavigationGraph  # noqa: F401
