"""knpemi -- MI355X-native hot path of the KNP-EMI solver (drop-in for `src/knpemi`).

Re-exports the twelve public names of the reference package (`src/knpemi/__init__.py:1-16`).  The reference's
`__all__` names several functions that do not exist; the list below is the set that can actually be imported
from it.  The device-resident loop of this implementation lives in `knpemi.stepper`; `Observables`
(`knpemi.observables`), `MembraneEvents` (`knpemi.events`), `IonFluxes` (`knpemi.fluxes`), `MembraneExchange`
(`knpemi.exchange`), `FieldMaps` (`knpemi.maps`), `MembraneMonitor` (`knpemi.monitor`) and `Snapshots`
(`knpemi.snapshots`: the fields themselves, packed on the device and written off the stepping thread) are its own additions: time
series of point values and field statistics, per-dof firing maps of the membranes, per-cell ion fluxes and current
densities with their integrals, what every ion carries across the membrane of a cell, with the mass budget it closes,
and per-vertex peak, arrival and exposure maps of phi, c and phi_M, and the membrane models' named intermediates
(Nernst potentials, currents by mechanism) at points, over a membrane and per dof.
"""
from .emiWeakForm import create_functions_emi, emi_system
from .events import MembraneEvents
from .exchange import MembraneExchange
from .fluxes import IonFluxes
from .maps import FieldMaps
from .monitor import MembraneMonitor
from .knpWeakForm import create_functions_knp, knp_system
from .observables import Observables
from .odeSolver import MembraneModel
from .pdeSolver import create_solver_emi, create_solver_knp
from .snapshots import Snapshots
from .utils import (interpolate_to_membrane, set_initial_conditions, setup_membrane_model, update_ode_variables,
                    update_pde_variables)

__all__ = sorted([
    "FieldMaps", "IonFluxes", "MembraneEvents", "MembraneExchange", "MembraneModel", "MembraneMonitor", "Observables", "Snapshots", "create_functions_emi", "create_functions_knp", "create_solver_emi", "create_solver_knp",
    "emi_system", "interpolate_to_membrane", "knp_system", "set_initial_conditions", "setup_membrane_model",
    "update_ode_variables", "update_pde_variables",
])
