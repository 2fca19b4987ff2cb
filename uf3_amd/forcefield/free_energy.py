"""
Anharmonic free energies by non-equilibrium thermodynamic integration (adiabatic switching; Freitas, Asta and de Koning,
Comput. Mater. Sci. 112, 333 (2016)), driven on the device by ``MolecularDynamics.switch``: ordinary molecular dynamics on
H(lambda) = K + lambda U_uf3 + (1 - lambda) U_E with lambda moving during the run, every replica, temperature and direction a
frame of one batch.

``frenkel_ladd``: the path between the model and an Einstein crystal gives F at one temperature,

    F = F_E (``einstein_free_energy``) + F_CM (``fixed_com_correction``) + Delta F,    Delta F = (W_forward - W_backward) / 2,

the dissipation (W_forward + W_backward) / 2 cancelling to first order.  ``reversible_scaling`` (de Koning, Antonelli and
Yip, PRL 83, 3973 (1999)): one run at T0 with the model's energy scaled by lambda gives F(T) for T = T0 / lambda.

Nuclei are classical.  Units: Angstrom, fs, amu, eV, K.  Everything above the two drivers is host arithmetic and needs no
device.

    out = frenkel_ladd(calc, atoms, 300.0, {'W': 183.84}, n_replicas=16)          # out['free_energy'], out['standard_error']
    curve = reversible_scaling(calc, atoms, 300.0, 1500.0, out['free_energy'], {'W': 183.84})
"""
import numpy as np

from uf3_amd.forcefield._driver import check_int, check_real
from uf3_amd.forcefield.md import ACC, KB

HBAR = 0.6582119569              # eV fs
WHO = "free_energy"


def switching_schedule(n_steps, kind="smooth"):
    """[n_steps + 1] the fraction of the way from the first to the last lambda at every state of a switch, from exactly 0 to
    exactly 1: ``"linear"``, tau = j / n_steps, or ``"smooth"``, Freitas's s(tau) = tau^5 (70 tau^4 - 315 tau^3 + 540 tau^2 -
    420 tau + 126), whose first four derivatives vanish at both ends (less dissipation where the switch starts and stops).
    ``n_steps`` = 0 gives [0]."""
    n = check_int(WHO, "n_steps", n_steps)
    if kind not in ("linear", "smooth"):
        raise ValueError(f"free_energy: schedule must be 'linear', 'smooth' or an array of n_steps + 1 values, got {kind!r}")
    if n == 0:
        return np.zeros(1)
    tau = np.arange(n + 1, dtype=float) / n
    s = tau if kind == "linear" else tau ** 5 * (70 * tau ** 4 - 315 * tau ** 3 + 540 * tau ** 2 - 420 * tau + 126)
    s = np.clip(s, 0.0, 1.0)
    s[0], s[-1] = 0.0, 1.0
    return np.ascontiguousarray(s)


def _spring_masses(spring, masses):
    k, m = np.asarray(spring, dtype=float).reshape(-1), np.asarray(masses, dtype=float).reshape(-1)
    if k.size == 1:
        k = np.full(m.size, k[0])
    if k.shape != m.shape or not k.size:
        raise ValueError(f"free_energy: {k.size} springs for {m.size} masses")
    if not (np.all(np.isfinite(k)) and np.all(k > 0) and np.all(np.isfinite(m)) and np.all(m > 0)):
        raise ValueError("free_energy: springs and masses must be positive and finite")
    return k, m


def einstein_free_energy(spring, masses, temperature_K):
    """Classical free energy of N independent three-dimensional oscillators, kT sum_i 3 ln(hbar omega_i / kT) in eV, with
    omega_i = sqrt(k_i ACC / m_i) in rad / fs (``spring`` eV / A^2, a scalar or per atom; ``masses`` amu) and hbar in eV fs."""
    k, m = _spring_masses(spring, masses)
    kt = KB * check_real(WHO, "temperature_K", temperature_K, strict=True)
    return float(kt * np.sum(3.0 * np.log(HBAR * np.sqrt(k * ACC / m) / kt)))


def fixed_com_correction(spring, masses, temperature_K, volume_A3, n_translations=None):
    """What holding the centre of mass fixed during the switch leaves out, in eV:

        F_CM = kT ln(n_translations / V) + (3 / 2) kT ln(2 pi kT sum_i mu_i^2 / k_i),    mu_i = m_i / M

    (Polson, Trizac, Pronk and Frenkel, J. Chem. Phys. 112, 5339 (2000), their general-mass form).  ``n_translations`` counts
    the translations that map the crystal onto itself inside ``volume_A3``: by default N for a frame of one species (every
    site is equivalent: a Bravais lattice or any cell given atom by atom of one kind) and 1 otherwise -- pass the number of
    primitive cells for a compound.  For one species, mu_i = 1 / N and k_i = m omega^2, this is Freitas, Asta and de Koning's
    F_CM = kT ln[(N / V) (2 pi kT / (N m omega^2))^(3/2)]."""
    k, m = _spring_masses(spring, masses)
    kt = KB * check_real(WHO, "temperature_K", temperature_K, strict=True)
    vol = check_real(WHO, "volume_A3", volume_A3, strict=True)
    if n_translations is None:
        n_translations = m.size if np.all(m == m[0]) and np.all(k == k[0]) else 1
    n_tr = check_int(WHO, "n_translations", n_translations, 1)
    mu = m / m.sum()
    return float(kt * np.log(n_tr / vol) + 1.5 * kt * np.log(2.0 * np.pi * kt * np.sum(mu * mu / k)))


def reversible_scaling_curve(work_so_far, lambdas, F0, T0, n_dof):
    """F(T) from a reversible-scaling run at ``T0``: with W(lambda) the reversible work of taking the energy's scale from 1
    to lambda (``work_so_far``, eV) and ``F0`` the free energy at T0,

        T = T0 / lambda,    F(T) = [F0 + W(lambda)] / lambda + (n_dof / 2) k_B T0 ln(lambda) / lambda,

    ``n_dof`` the momenta that move (3 N - 3 with the centre of mass held).  Returns (T, F)."""
    w, lam = np.asarray(work_so_far, dtype=float), np.asarray(lambdas, dtype=float)
    if w.shape != lam.shape:
        raise ValueError(f"free_energy: work_so_far {list(w.shape)} and lambdas {list(lam.shape)} differ in shape")
    if not np.all(np.isfinite(lam)) or np.any(lam <= 0):
        raise ValueError("free_energy: lambdas must be positive and finite")
    t0 = check_real(WHO, "T0", T0, strict=True)
    n_dof = check_int(WHO, "n_dof", n_dof, 1)
    return t0 / lam, (float(F0) + w) / lam + 0.5 * n_dof * KB * t0 * np.log(lam) / lam


def spring_constants(dyn, n_steps, msd_every=10):
    """Per-species springs k_s = 3 k_B T / <|dr|^2>_s in eV / A^2 from ``n_steps`` of ``dyn.run`` at its temperature: the
    mean-squared displacement from the MSD origin (``dyn.set_msd_origin``: give it the lattice sites, or call this on an
    object that still sits on them) with the centre-of-mass displacement removed (``msd_com_removed``), averaged over the
    second half of the samples and over the frames.  Returns ``{symbol: k}`` for the species present."""
    n_steps = check_int(WHO, "n_steps", n_steps, 1)
    msd_every = check_int(WHO, "msd_every", msd_every, 1, n_steps)
    temp = check_real(WHO, "temperature_K", dyn.temperature_K, strict=True)
    rec = dyn.run(n_steps, msd_every=msd_every)
    msd = rec["msd_com_removed"]
    msd = msd[len(msd) // 2:]
    elements = dyn.calculator.bspline_config.chemical_system.element_list
    out = {}
    for s, el in enumerate(elements):
        col = msd[:, :, s]
        if np.all(np.isnan(col)):
            continue
        out[el] = float(3.0 * KB * temp / np.nanmean(col))
    return out


def _replica_batch(atoms, temperatures, n_replicas):
    temps = np.atleast_1d(np.asarray(temperatures, dtype=float))
    if temps.ndim != 1 or not temps.size or not np.all(np.isfinite(temps)) or np.any(temps <= 0):
        raise ValueError(f"free_energy: temperatures must be positive and finite, got {temperatures!r}")
    n_rep = check_int(WHO, "n_replicas", n_replicas, 1)
    return temps, n_rep, [atoms] * (n_rep * temps.size), np.repeat(temps, n_rep)


def frenkel_ladd(calc, atoms, temperature_K, masses=None, n_replicas=8, n_equilibrate=1000, n_switch=3000, spring=None,
                 timestep_fs=1.0, friction_per_fs=0.02, seed=0, schedule="smooth", skin=0.5, n_spring=2000, n_translations=None):
    """Free energy of the crystal ``atoms`` (sitting on its lattice sites) at ``temperature_K`` -- a number or a list; the
    ``n_replicas`` replicas of every temperature form one batch -- by Frenkel-Ladd switching with the centre of mass held:
    equilibrate ``n_equilibrate`` steps at lambda = 0 (the Einstein crystal), switch to 1 (the model) in ``n_switch`` steps,
    equilibrate there, switch back.  ``spring`` as ``MolecularDynamics.set_reference`` takes it; None measures it first with
    ``spring_constants`` (``n_spring`` Langevin steps at the first temperature).  Returns a dict, arrays over the temperatures:
    ``temperature``, ``free_energy`` = F_E + F_CM + mean Delta F (eV per cell), ``standard_error`` of that mean, ``delta_F``
    and ``dissipation`` [n_T, n_replicas], ``work_forward``, ``work_backward``, ``einstein_free_energy``,
    ``com_correction`` and ``spring`` [N]."""
    from uf3_amd.forcefield.md import MolecularDynamics
    temps, n_rep, frames, per_frame = _replica_batch(atoms, temperature_K, n_replicas)
    n_eq = check_int(WHO, "n_equilibrate", n_equilibrate)
    n_sw = check_int(WHO, "n_switch", n_switch, 1)
    common = dict(masses=masses, friction_per_fs=check_real(WHO, "friction_per_fs", friction_per_fs, strict=True), seed=seed, skin=skin)
    if spring is None:
        with MolecularDynamics(calc, [atoms], timestep_fs, temperature_K=float(temps[0]), **common) as probe:
            probe.initialize_velocities(float(temps[0]))
            spring = spring_constants(probe, check_int(WHO, "n_spring", n_spring, 2), msd_every=max(1, min(10, n_spring // 2)))
    with MolecularDynamics(calc, frames, timestep_fs, temperature_K=float(temps[0]), **common) as dyn:
        n_atoms = len(atoms)
        dyn.set_reference(None, spring)
        k, m = dyn.spring[:n_atoms].copy(), dyn.masses[:n_atoms].copy()
        volume = float(dyn.volumes[0])
        dyn.initialize_velocities(float(temps[0]))
        work = {}
        for name, a, b in (("forward", 0.0, 1.0), ("backward", 1.0, 0.0)):
            dyn.switch(n_eq, a, a, temperatures_K=per_frame)
            work[name] = dyn.switch(n_sw, a, b, schedule=schedule, temperatures_K=per_frame)["work"].reshape(temps.size, n_rep)
    if not volume > 0:
        raise ValueError("free_energy: the frame has no volume: the centre-of-mass correction needs a periodic cell")
    delta = 0.5 * (work["forward"] - work["backward"])
    f_e = np.array([einstein_free_energy(k, m, t) for t in temps])
    f_cm = np.array([fixed_com_correction(k, m, t, volume, n_translations) for t in temps])
    se = delta.std(axis=1, ddof=1) / np.sqrt(n_rep) if n_rep > 1 else np.full(temps.size, np.nan)
    return dict(temperature=temps, free_energy=f_e + f_cm + delta.mean(axis=1), standard_error=se, delta_F=delta,
                dissipation=0.5 * (work["forward"] + work["backward"]), work_forward=work["forward"],
                work_backward=work["backward"], einstein_free_energy=f_e, com_correction=f_cm, spring=k)


def reversible_scaling(calc, atoms, T0, T1, F0, masses=None, n_replicas=8, n_equilibrate=1000, n_switch=3000, n_points=100,
                       timestep_fs=1.0, friction_per_fs=0.02, seed=0, schedule="linear", skin=0.5):
    """F(T) between ``T0`` and ``T1`` >= T0 from one pair of switches at T0 in which the model's energy is scaled by lambda
    from 1 to T0 / T1 and back (no spring: ``set_reference(spring=None)``), the centre of mass held; ``F0`` is the free energy
    at T0 (``frenkel_ladd``'s).  The reversible work at each of ``n_points`` values of lambda is half the difference of the
    forward work so far and the backward work still to come, averaged over ``n_replicas``; the schedule must be symmetric
    (both named ones are).  Returns ``temperature``, ``free_energy`` (``reversible_scaling_curve``), ``lambda``, ``work`` and
    ``dissipation`` (per replica, of the whole switch)."""
    from uf3_amd.forcefield.md import MolecularDynamics
    t0, t1 = check_real(WHO, "T0", T0, strict=True), check_real(WHO, "T1", T1, strict=True)
    if t1 < t0:
        raise ValueError("free_energy: T1 must be >= T0 (the scale lambda = T0 / T lies in (0, 1])")
    _, n_rep, frames, _ = _replica_batch(atoms, t0, n_replicas)
    n_eq, n_pts = check_int(WHO, "n_equilibrate", n_equilibrate), check_int(WHO, "n_points", n_points, 1)
    n_sw = check_int(WHO, "n_switch", n_switch, 1)
    every = max(1, n_sw // n_pts)
    n_sw -= n_sw % every                                        # (the two directions' records then meet at the same lambdas)
    lam_end = t0 / t1
    with MolecularDynamics(calc, frames, timestep_fs, masses=masses, temperature_K=t0,
                           friction_per_fs=check_real(WHO, "friction_per_fs", friction_per_fs, strict=True), seed=seed, skin=skin) as dyn:
        dyn.set_reference(None, None)
        dyn.initialize_velocities(t0)
        dyn.switch(n_eq, 1.0, 1.0)
        fwd = dyn.switch(n_sw, 1.0, lam_end, schedule=schedule, every=every)
        dyn.switch(n_eq, lam_end, lam_end)
        bwd = dyn.switch(n_sw, lam_end, 1.0, schedule=schedule, every=every)
    # backward work so far at the lambda of forward record r: the record n_rec - 2 - r steps in, nothing at the start
    back_so_far = np.concatenate([np.zeros((1, n_rep)), bwd["work_so_far"]])[::-1][1:]
    work = 0.5 * (fwd["work_so_far"] - (bwd["work"][None] - back_so_far))
    lam = fwd["lambda"][:, 0]
    temperature, free = reversible_scaling_curve(work.mean(axis=1), lam, F0, t0, 3 * len(atoms) - 3)
    return {"temperature": temperature, "free_energy": free, "lambda": lam, "work": work,
            "dissipation": 0.5 * (fwd["work"] + bwd["work"])}
