"""Shared test helpers.  abi_cases holds one case per stream-taking entry point of include/pinsage_hip.h in its CASES table; the
cases of entry points added since live in modules of their own, which register themselves in that table when imported.  They are
imported here, so whoever imports anything from `helpers` sees the whole table."""
from . import abi_cases_linear_bwd  # noqa: F401  (ps_linear_wgrad, ps_linear_epilogue_bwd)
