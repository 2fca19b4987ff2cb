"""
Pair-distance histograms of a training set, for choosing cut-offs: the public surface of the reference's
``uf3/data/analyze.py`` (``DataAnalyzer`` and the module functions), same names, signatures and results.

The reference takes ``scipy.spatial.distance.cdist`` of every frame against its explicit supercell (27 x 10 000 atoms for a
10 000-atom frame at 12 A: a 21.6 GB matrix) and bins the masked distances with ``np.histogram``.  Here the counting is
``libuf3hip.so``'s ``uf3_pair_histogram``: the cell list of the featurizer enumerates the same (centre, image) pairs, in the
reference's arithmetic, and a kernel bins them; frames go to the device in batches bounded by an atom count.  What follows
the counts -- normalisation, smoothing, peak finding, the volume regression -- is the reference's host post-processing
(scipy / scikit-learn), kept with its quirks: ``analyze()`` re-keys the Szudzik pair hashes to symbol tuples, and a pair of
the chemical system that was never observed raises ``KeyError`` there.

Without the library / a gfx950 device, every call that counts raises ``uf3_amd._lib.HipUnavailable``.
"""
import warnings
from typing import Any, Dict, Tuple, Union

import numpy as np
from scipy import optimize as sp_opt
from scipy import signal
from sklearn import linear_model as sk_linear

from uf3_amd import _lib
from uf3_amd.data import composition

# frames per device call: as many as fit under this many atoms (a frame larger than it goes alone)
MAX_BATCH_ATOMS = 400_000


# ------------------------------------------------------------------------------ post-processing (host)
def get_uniform_normalization(bins, n_atoms, volume):
    """Pair counts per bin of an ideal gas of ``n_atoms`` atoms in ``volume``: shell volumes over the volume per atom,
    times the number of atoms."""
    r_lo, r_hi = bins[:-1], bins[1:]
    per_atom = volume / n_atoms
    shell = 4 / 3 * np.pi * (r_hi ** 3) - 4 / 3 * np.pi * (r_lo ** 3)
    return shell / per_atom * n_atoms


def apply_binning(dist_ref, bins):
    """{key: np.histogram(distances, bins) counts}."""
    return {key: np.histogram(values, bins)[0] for key, values in dist_ref.items()}


def score_coverage(x, histogram, reference, weight=10):
    """Loss of a reference density scaled by ``x`` against the histogram: minus (reference mass under the histogram, past
    the first observed bin) minus ``weight`` times the overshoot (Nelder-Mead minimises it in ``DataAnalyzer.analyze``)."""
    histogram = np.array(histogram)
    first = np.where(np.nonzero(histogram))[0][0]
    scaled = reference * x
    gap = histogram - scaled
    under = scaled[gap >= 0][first:]
    over = gap[gap < 0][first:]
    return -(np.sum(under) + np.sum(over * weight))


def compute_coverage(x, histogram, reference):
    """Area of the histogram under the reference density scaled by ``x``."""
    excess = histogram - reference * x
    excess[excess < 0] = 0
    return np.sum(histogram - excess)


def suggest_cutoffs(lower_bound, valley_list, bond_length):
    print(f"    Smallest observed: {lower_bound:.2f} angstroms")
    print("    Suggested Cutoffs:", valley_list[valley_list >= bond_length])


def find_peaks(x, y, smooth=False, filter_width=9, filter_degree=3):
    """Indices and positions of the local maxima of ``y`` (Savitzky-Golay smoothed first with ``smooth``)."""
    if smooth:
        y = signal.savgol_filter(y, filter_width, filter_degree)
    idx = signal.find_peaks(y)[0]
    return idx, x[idx]


def find_closest_value(values, target):
    idx = np.argmin(np.abs(values - target))
    return idx, values[idx]


# ------------------------------------------------------------------------------ device counting
def _pair_hash(za, zb):
    """Szudzik hash of a species pair sorted by atomic number (composition.get_pair_hashes)."""
    lo, hi = min(za, zb), max(za, zb)
    return int(hi * hi + lo + hi)


_bases = {}


def _hist_basis(species_z, r_min, r_max):
    """RawDeviceBasis with every pair of ``species_z`` at (r_min, r_max) and the supercell range r_max (cached)."""
    ctx = _lib.get_context()
    key = (id(ctx), tuple(species_z), float(r_min), float(r_max))
    b = _bases.get(key)
    if b is None:
        zs = list(species_z)
        pairs = {(zs[i], zs[j]): (float(r_min), float(r_max)) for i in range(len(zs)) for j in range(i, len(zs))}
        b = _bases[key] = _lib.RawDeviceBasis(zs, pairs, r_cut=float(r_max), ctx=ctx)
    return b


def _noise_table(stdev, n_rows):
    """ASE's rattle noise for the first ``n_rows`` supercell atoms: RandomState(42).normal is a prefix-stable stream, so one
    table serves every frame, indexed by reference supercell index."""
    return np.random.RandomState(42).normal(scale=stdev, size=(int(n_rows), 3))


def _supercell_size(geom, r_cut):
    from uf3_amd.data import geometry
    pbc = np.asarray(geom.get_pbc() if hasattr(geom, "get_pbc") else geom.pbc, dtype=bool)
    if not pbc.any():
        return len(geom)
    return len(geometry.image_shifts(np.asarray(geom.get_cell(), dtype=float).reshape(3, 3), pbc, r_cut)) * len(geom)


def _batches(geometries, max_atoms=MAX_BATCH_ATOMS):
    batch, n = [], 0
    for g in geometries:
        if batch and n + len(g) > max_atoms:
            yield batch
            batch, n = [], 0
        batch.append(g)
        n += len(g)
    if batch:
        yield batch


def pair_histograms(geometries, species_z, bin_edges, r_min=0.0, r_max=12.0, upper_inclusive=True, rattle=0.0,
                    per_frame=False, max_atoms=MAX_BATCH_ATOMS):
    """Counts of every ordered (centre, supercell image) pair with r_min < d <= r_max (``upper_inclusive``) or
    r_min < d < r_max, per species pair of ``species_z`` (ascending atomic numbers, every element of the frames among them)
    and bin of ``bin_edges``: int64 [P][n_bins] summed over the frames, or [n_frames][P][n_bins] with ``per_frame``; pairs
    in the order (z_i, z_j), i <= j.  Periodic frames meet their supercell of range r_max; ``rattle`` > 0 moves that
    supercell by ASE's ``rattle(rattle)`` noise (the centres stay).  Non-periodic frames are compared with themselves as
    given (the caller rattles them)."""
    geometries = list(geometries)
    dbasis = _hist_basis(species_z, r_min, r_max)
    edges = np.ascontiguousarray(bin_edges, dtype=np.float64)
    n_pairs, n_bins = len(dbasis.pairs), len(edges) - 1
    out = np.zeros(((len(geometries),) if per_frame else ()) + (n_pairs, n_bins), dtype=np.int64)
    periodic = [bool(np.any(g.get_pbc() if hasattr(g, "get_pbc") else g.pbc)) for g in geometries]
    start = 0
    for batch in _batches(geometries, max_atoms):
        idx = np.arange(start, start + len(batch))
        start += len(batch)
        for want_pbc in (True, False):
            sel = [k for k in idx if periodic[k] == want_pbc]
            if not sel:
                continue
            frames = [geometries[k] for k in sel]
            noise = None
            if rattle > 0 and want_pbc:
                noise = _noise_table(rattle, max(_supercell_size(g, r_max) for g in frames))
            fb = _lib.FrameBatch(frames)
            counts = _lib.pair_histogram(dbasis, fb, edges, upper_inclusive=upper_inclusive, noise=noise,
                                         per_frame=per_frame)
            if per_frame:
                out[np.asarray(sel)] = counts
            else:
                out += counts
    return out, list(dbasis.pairs)


# ------------------------------------------------------------------------------ DataAnalyzer
class DataAnalyzer:
    def __init__(self,
                 chemical_system: composition.ChemicalSystem,
                 r_cut: float = 12.0,
                 rattle: float = 0.0,
                 bins: Union[int, float] = 0.01,
                 min_peak_width: float = 0.2,
                 progress: Any = "bar"):
        """
        Args:
            chemical_system (ChemicalSystem)
            r_cut (float): cutoff distance in angstroms.
            rattle: amplitude of ASE's rattle applied to the neighbours (supercell) of periodic frames, or to the frame
                itself (in place) for clusters: broadens the peaks of the distribution.
            bins (int, float): int: number of bins; float: bin width in angstroms.
            min_peak_width (float): minimum peak width in angstroms.
            progress: accepted for compatibility; no progress bar is drawn.
        """
        self.chemical_system = chemical_system
        self.r_cut = r_cut
        self.rattle = rattle
        self.min_peak_width = min_peak_width
        self.progress = progress
        self.element_set = chemical_system.numbers
        self.element_names = chemical_system.element_list
        self.n_elements = len(self.element_set)
        self.pair_tuples = chemical_system.interactions_map[2]
        self.n_bins = bins if isinstance(bins, int) else int(np.ceil(r_cut / bins))
        self.bin_edges = np.linspace(0, r_cut, self.n_bins + 1)
        self.bin_width = np.mean(self.bin_edges[1::2] - self.bin_edges[:-1:2])
        self.bin_centers = 0.5 * np.add(self.bin_edges[:-1], self.bin_edges[1:])
        self.bin_span = int(np.ceil(min_peak_width / self.bin_width))
        self.clear()
        self.outliers = {}

    def clear(self):
        """Reset accumulated pair and volume data."""
        self.histogram_values = {}
        self.pairs_acc = {}
        self.totals_acc = 0
        self.sizes = []
        self.volumes = []
        self.compositions = []
        self.lower_bounds = {}
        self.peaks = {}
        self.valleys = {}
        self.volume_ref = {}
        self.radii_ref = {}
        self.density_ref = {}
        self.normalized_values = {}

    def _record(self, geom):
        numbers = np.asarray(geom.get_atomic_numbers())
        if any(n not in self.element_set for n in numbers):
            warnings.warn(f"Invalid element detected: {numbers}")
        self.sizes.append(len(geom))
        self.volumes.append(geom.get_volume())
        self.compositions.append([np.count_nonzero(numbers == el) for el in self.element_set])

    def _count(self, geometries, r_min, r_max, rattle):
        """Histograms of a list of frames on the device, added to the accumulators (keys in ascending hash order)."""
        species = sorted(set(int(z) for z in self.element_set)
                         | set(int(z) for g in geometries for z in np.unique(g.get_atomic_numbers())))
        if rattle > 0:
            for g in geometries:
                if not np.any(g.get_pbc() if hasattr(g, "get_pbc") else g.pbc):
                    g.rattle(rattle)            # clusters: the reference rattles the caller's frame in place
        counts, pairs = pair_histograms(geometries, species, self.bin_edges, r_min, r_max, upper_inclusive=True,
                                        rattle=rattle)
        by_hash = sorted((_pair_hash(za, zb), p) for p, (za, zb) in enumerate(pairs))
        for key, p in by_hash:
            n_pairs = counts[p].sum()
            if n_pairs == 0:
                continue
            if key not in self.histogram_values:
                self.histogram_values[key] = np.zeros(self.n_bins)
                self.pairs_acc[key] = 0
            self.histogram_values[key] += counts[p]
            self.pairs_acc[key] += n_pairs
            self.totals_acc += n_pairs

    def process_geometry(self, geom, r_min: float = None, r_max: float = None, rattle: float = None):
        """Add the pair-distance histograms of one frame."""
        r_min = 0.0 if r_min is None else r_min
        r_max = self.r_cut if r_max is None else r_max
        rattle = self.rattle if rattle is None else rattle
        self._record(geom)
        self._count([geom], r_min, r_max, rattle)

    def update_histograms(self, dist_ref):
        """Add {pair hash: distances} binned on ``bin_edges`` (the reference's host route for given distances)."""
        for key, hist in apply_binning(dist_ref, self.bin_edges).items():
            n_pairs = np.sum(hist)
            if key not in self.histogram_values:
                self.histogram_values[key] = np.zeros(self.n_bins)
                self.pairs_acc[key] = 0
            self.histogram_values[key] += hist
            self.pairs_acc[key] += n_pairs
            self.totals_acc += n_pairs

    def load_entries(self, geometries):
        """Add the histograms of every frame: one device call per batch of frames of up to MAX_BATCH_ATOMS atoms."""
        geometries = list(geometries)
        for g in geometries:
            self._record(g)
        for batch in _batches(geometries):
            self._count(batch, 0.0, self.r_cut, self.rattle)

    def normalize_pair_histogram(self, pair, n_atoms, volume):
        norm = get_uniform_normalization(self.bin_edges, n_atoms, volume)
        weight = self.pairs_acc[pair] / self.totals_acc
        return norm, self.histogram_values[pair] / norm / weight

    def analyze(self, smooth: bool = True, filter_width: int = 9, filter_degree: int = 3) -> Dict:
        """Normalised distributions, coverage, peaks, valleys and suggested cut-offs per pair."""
        reference, rdfs, coverages, factors = {}, {}, {}, {}
        if any(isinstance(k, int) for k in self.pairs_acc):
            to_symbols = {k: composition.hash_to_symbols(k) for k in self.histogram_values}
            self.pairs_acc = {to_symbols[k]: v for k, v in self.pairs_acc.items()}
            self.histogram_values = {to_symbols[k]: v for k, v in self.histogram_values.items()}
        atomic_volumes, _ = self.fit_element_data()
        bond_ref = {pair: (np.mean([atomic_volumes[el] for el in pair]) / (4 / 3 * np.pi)) ** (1 / 3) * 2
                    for pair in self.pair_tuples}
        n_atoms = np.sum(self.sizes)
        volume = np.sum(self.volumes)
        for pair in self.pair_tuples:
            hist = self.histogram_values[pair]
            if np.sum(hist) == 0:
                warnings.warn(f"No observed {pair} pairs.")
                continue
            norm, rdf = self.normalize_pair_histogram(pair, n_atoms, volume)
            rdfs[pair] = rdf
            reference[pair] = norm
            scale = sp_opt.minimize(score_coverage, 1, args=(hist, norm, 10), method="Nelder-Mead").x
            coverages[pair] = compute_coverage(scale, hist, norm)
            self.find_pair_distribution_peaks(pair, smooth=smooth, filter_width=filter_width,
                                              filter_degree=filter_degree)
            suggest_cutoffs(self.lower_bounds[pair], self.valleys[pair], bond_ref[pair])
        return dict(histograms=self.histogram_values, bin_edges=self.bin_edges, reference=reference, rdfs=rdfs,
                    coverage=coverages, factors=factors, lower_bounds=self.lower_bounds, peaks=self.peaks,
                    valleys=self.valleys, atomic_volumes=atomic_volumes)

    def fit_element_data(self):
        """Volume per atom of each element: Huber regression of the frame volumes on the compositions (with a tiny ridge
        block of rows)."""
        x = np.concatenate([self.compositions, np.ones((self.n_elements, self.n_elements)) * 1e-6])
        y = np.concatenate([self.volumes, np.zeros(self.n_elements)])
        regr = sk_linear.HuberRegressor(fit_intercept=False)
        regr.fit(x, y)
        soln = regr.coef_
        return dict(zip(self.element_names, soln)), soln

    def find_pair_distribution_peaks(self, pair: Tuple, smooth: bool = True, filter_width: int = 9,
                                     filter_degree: int = 3):
        hist = self.histogram_values[pair]
        self.lower_bounds[pair] = self.bin_edges[np.nonzero(hist)[0][0]]
        _, peak_list = find_peaks(self.bin_centers, hist, smooth=smooth, filter_width=filter_width,
                                  filter_degree=filter_degree)
        self.valleys[pair] = np.mean([peak_list[1:], peak_list[:-1]], axis=0)
        self.peaks[pair] = peak_list
