"""The entry-wise reference of the FAST operators (CPU only, numpy, fp64): shared by tests/test_operator_probe_host.py,
tests/test_gpu_operator_probe.py and tests/test_gpu_pcg_identities.py.

Reference operator. K_ref = s_K sum_e Ke + s_M diag(m) with plain fp64 element matrices:
  tet4  Ke = V B^T D B from the packed f32 gradients and volumes widened (the operator the handle holds, as
        test_gpu_refine.dense takes it);
  hex8  trilinear, full 2 x 2 x 2 Gauss, from the fp64 coordinates (corners in Gmsh / VTK order).
Voigt order xx, yy, zz, xy, yz, xz with engineering shear. The Dirichlet rule is the oracle's (orc_apply_keff,
hex8_apply_impl): a constrained row passes x through, a constrained column is dropped. Next to K_ref the class holds
the element-wise absolute assembly A = s_K sum_e |Ke| + |s_M| diag(m), the scale every bound is written in:

  R_I      the largest diagonal entry of A over the three rows of node I (the entry scale of node I's rows);
  A |x|    the component-wise scale of a product.

Probe vectors. Unit vectors recover a matrix column by column. On a box lattice the 27 colours (i mod 3, j mod 3,
k mod 3) times the three components give 81 vectors with 1.0 at every node of one colour: two nodes of one colour are
at least three apart along an axis, so no row (its reach is one cell) sees more than one of them and each product entry
is one matrix entry. Which rows a probe can reach at all (its structural non-zeros) is decided from the connectivity.

u = 2^-24 is the unit roundoff of fp32.
"""
import numpy as np

U = 2.0 ** -24
DOF_BITS = np.array([1, 2, 4], np.uint32)
_GAUSS = 1.0 / np.sqrt(3.0)
_HEX_SIGN = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
                      [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)


def stiffness_array(materials):
    """[M, 6, 6] fp64 from ElasticProperties records or plain 36-vectors / 6 x 6 arrays."""
    return np.stack([np.asarray(m.stiffness if hasattr(m, "stiffness") else m, np.float64).reshape(6, 6)
                     for m in materials])


def _strain_matrix(g):
    """B [E, 6, 3 n] of the shape-function gradients g [E, n, 3]."""
    E, n, _ = g.shape
    B = np.zeros((E, 6, n, 3))
    gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
    B[:, 0, :, 0] = gx
    B[:, 1, :, 1] = gy
    B[:, 2, :, 2] = gz
    B[:, 3, :, 0], B[:, 3, :, 1] = gy, gx
    B[:, 4, :, 1], B[:, 4, :, 2] = gz, gy
    B[:, 5, :, 0], B[:, 5, :, 2] = gz, gx
    return B.reshape(E, 6, 3 * n)


def tet4_element_matrices(gradients, volume, material_index, D):
    """Ke [E, 12, 12] = V B^T D B; gradients f32 [E * 24] (the first 12 of an element: four corners x 3), volume f32."""
    E = np.asarray(volume).size
    g = np.asarray(gradients).reshape(E, -1)[:, :12].astype(np.float64).reshape(E, 4, 3)
    B = _strain_matrix(g)
    DB = np.einsum("eij,ejk->eik", D[np.asarray(material_index, np.int64)], B)
    return np.einsum("eri,erj->eij", B, DB) * np.asarray(volume, np.float64)[:, None, None]


def hex8_element_matrices(coords, hexes, material_index, D):
    """Ke [E, 24, 24] = sum over the 8 Gauss points of |det J| B^T D B (weights 1 on [-1, 1]^3)."""
    X = np.asarray(coords, np.float64)[np.asarray(hexes, np.int64).reshape(-1, 8)]  # [E, 8, 3]
    E = X.shape[0]
    De = D[np.asarray(material_index, np.int64)]
    Ke = np.zeros((E, 24, 24))
    for p in range(8):
        q = np.array([_GAUSS if p & 1 else -_GAUSS, _GAUSS if p & 2 else -_GAUSS, _GAUSS if p & 4 else -_GAUSS])
        f = 1.0 + _HEX_SIGN * q  # [8, 3]
        dN = 0.125 * np.stack([_HEX_SIGN[:, 0] * f[:, 1] * f[:, 2], f[:, 0] * _HEX_SIGN[:, 1] * f[:, 2],
                               f[:, 0] * f[:, 1] * _HEX_SIGN[:, 2]], 1)  # dN_a / dxi_l
        J = np.einsum("eam,al->eml", X, dN)  # dx_m / dxi_l
        g = np.einsum("al,elm->eam", dN, np.linalg.inv(J))  # dN_a / dx_m
        B = _strain_matrix(g)
        DB = np.einsum("eij,ejk->eik", De, B)
        Ke += np.einsum("eri,erj->eij", B, DB) * np.abs(np.linalg.det(J))[:, None, None]
    return Ke


class Reference:
    """K_ref and A of one mesh, matrix-free over blocks of vectors. conn [E, n] node ids, Ke [E, 3 n, 3 n] (s_K not
    applied), mass the f32 lumped mass, bc_mask the per-node axis bits."""

    def __init__(self, conn, Ke, mass, bc_mask, sK, sM):
        self.conn = np.asarray(conn, np.int64)
        E, n = self.conn.shape
        self.N = int(np.asarray(bc_mask).size)
        self.D = 3 * self.N
        self.Ke = np.asarray(Ke, np.float64) * float(sK)
        self.m = np.repeat(np.asarray(mass, np.float32).astype(np.float64), 3) * float(sM)
        self.fixed = (np.repeat(np.asarray(bc_mask, np.uint32), 3) & np.tile(DOF_BITS, self.N)) != 0
        self.free = ~self.fixed
        self.dofs = (3 * self.conn[:, :, None] + np.arange(3)[None, None, :]).reshape(E, 3 * n)
        flat = self.dofs.reshape(-1)
        self._order = np.argsort(flat, kind="stable")
        self._rows, self._starts = np.unique(flat[self._order], return_index=True)
        kd = np.abs(np.einsum("eii->ei", self.Ke)).reshape(-1)
        self.diag_abs = np.abs(self.m).copy()
        np.add.at(self.diag_abs, flat, kd)
        self.node_scale = self.diag_abs.reshape(self.N, 3).max(1)  # R_I
        self.row_scale = np.repeat(self.node_scale, 3)  # R_I per DOF

    def _assemble(self, Ke, mdiag, V, chunk=64):
        V = np.asarray(V, np.float64)
        one = V.ndim == 1
        V = V.reshape(self.D, -1)
        Y = np.zeros_like(V)
        E, nd = self.dofs.shape
        for c in range(0, V.shape[1], chunk):
            W = V[:, c:c + chunk]
            F = np.einsum("eij,ejm->eim", Ke, W[self.dofs]).reshape(E * nd, -1)
            Y[self._rows, c:c + chunk] = np.add.reduceat(F[self._order], self._starts, axis=0)
        Y += mdiag[:, None] * V
        return Y[:, 0] if one else Y

    def apply(self, V):
        """K_ref @ V for V [D] or [D, m], with the Dirichlet rule."""
        V = np.asarray(V, np.float64)
        fx = self.fixed if V.ndim == 1 else self.fixed[:, None]
        Y = self._assemble(self.Ke, self.m, np.where(fx, 0.0, V))
        return np.where(fx, V, Y)

    def apply_abs(self, V):
        """A @ |V| under the same rule (a constrained row gives |x|)."""
        V = np.abs(np.asarray(V, np.float64))
        fx = self.fixed if V.ndim == 1 else self.fixed[:, None]
        Y = self._assemble(np.abs(self.Ke), np.abs(self.m), np.where(fx, 0.0, V))
        return np.where(fx, V, Y)

    def dense(self):
        """K_ref [D, D] (columns of the identity); small meshes only."""
        return self.apply(np.eye(self.D))

    def reach(self, probe_nodes):
        """bool [N]: the nodes that share an element with a node of `probe_nodes` (bool [N] or [N, m]), from the
        connectivity alone. Rows of every other node are structural zeros of the probe."""
        pn = np.asarray(probe_nodes, bool)
        one = pn.ndim == 1
        pn = pn.reshape(self.N, -1)
        out = np.zeros_like(pn)
        for c in range(pn.shape[1]):
            hit = pn[self.conn, c].any(1)
            out[self.conn[hit].reshape(-1), c] = True
        return out[:, 0] if one else out


def tet4_reference(P, materials, sK, sM, material_index=None, bc_mask=None):
    """Reference of a tet4 packing (cwf.pack.PackingResult)."""
    E = int(P.element_count)
    mi = P.material_index if material_index is None else material_index
    Ke = tet4_element_matrices(P.gradients, P.volume, mi, stiffness_array(materials))
    conn = np.asarray(P.connectivity).reshape(E, -1)[:, :4]
    return Reference(conn, Ke, P.lumped_mass, P.bc_mask if bc_mask is None else bc_mask, sK, sM)


def hex8_reference(case, materials, sK, sM, material_index=None, bc_mask=None):
    P = case.packing
    mi = P.material_index if material_index is None else material_index
    Ke = hex8_element_matrices(case.mesh.coords, case.mesh.tets, mi, stiffness_array(materials))
    return Reference(np.asarray(case.mesh.tets).reshape(-1, 8), Ke, P.lumped_mass,
                     P.bc_mask if bc_mask is None else bc_mask, sK, sM)


def is_hex(case):
    return np.asarray(case.mesh.tets).shape[1] == 8


def reference_of(case, materials=None, scalars=None, material_index=None, bc_mask=None):
    """Reference of a scenarios.Case (or materials_common.MaterialCase), tet4 or hex8 by its connectivity; bc_mask
    overrides the packing's (the handle without Dirichlet nodes)."""
    materials = case.materials if materials is None else materials
    sK, sM = case.scalars() if scalars is None else scalars
    if is_hex(case):
        return hex8_reference(case, materials, sK, sM, material_index, bc_mask)
    return tet4_reference(case.packing, materials, sK, sM, material_index, bc_mask)


# ---- probe vectors ---------------------------------------------------------------------------------------------------
def lattice_index(coords):
    """(i, j, k) [N, 3] of the nodes of a box lattice in any node order, from the coordinates."""
    c = np.asarray(coords, np.float64)
    span = float((c.max(0) - c.min(0)).max())
    return np.stack([np.unique(np.round(c[:, a] / span * 2 ** 20), return_inverse=True)[1].reshape(-1)
                     for a in range(3)], 1)


def colour_probes(colour, ncolours):
    """(V f32 [D, 3 ncolours], probe_nodes bool [N, 3 ncolours], component [3 ncolours]): vector 3 c + a has 1.0 at
    component a of every node of colour c."""
    colour = np.asarray(colour, np.int64)
    N = colour.size
    V = np.zeros((N, 3, ncolours, 3), np.float32)
    for a in range(3):
        V[np.arange(N), a, colour, a] = 1.0
    nodes = np.repeat(colour[:, None] == np.arange(ncolours)[None, :], 3, 1)
    return V.reshape(3 * N, 3 * ncolours), nodes, np.tile(np.arange(3), ncolours)


def lattice_probes(coords):
    """The 81 coloured probes of a box lattice."""
    ijk = lattice_index(coords) % 3
    return colour_probes(ijk[:, 0] + 3 * ijk[:, 1] + 9 * ijk[:, 2], 27)


def unit_probes(N):
    """All 3 N unit vectors (every node its own colour)."""
    return colour_probes(np.arange(N), N)


def banded_probes(D, half_bandwidth):
    """f32 [D, 2 hb + 1]: vector c has 1.0 at every index = c mod (2 hb + 1); recovers a matrix of that band."""
    w = 2 * half_bandwidth + 1
    return (np.arange(D)[:, None] % w == np.arange(w)[None, :]).astype(np.float32)


def read_banded(Y, half_bandwidth):
    """The banded matrix [D, D] whose products with banded_probes are Y [D, w]."""
    D, w = Y.shape
    M = np.zeros((D, D))
    for i in range(D):
        for j in range(max(0, i - half_bandwidth), min(D, i + half_bandwidth + 1)):
            M[i, j] = Y[i, j % w]
    return M


# ---- the checks ------------------------------------------------------------------------------------------------------
def probe_report(ref, V, probe_nodes, component, Y, Yref=None):
    """What a block of probe products Y = K_fast V shows against the reference, as counts and ratios (no assertion):
      structural   entries that are not +-0.0 on rows of nodes out of the probe's reach
      passthrough  constrained rows that differ from x
      leaked       free rows in reach of constrained probe DOFs only that are not +-0.0 (coloured probes put at most
                   one probe node in a row's reach, so such a row sees nothing else)
      entry        max |Y - K_ref V|_i / (u R_I) over the free rows
    """
    V = np.asarray(V)
    Y = np.asarray(Y)
    Yref = ref.apply(V) if Yref is None else Yref
    reach = np.repeat(ref.reach(probe_nodes), 3, 0)  # [D, m]
    free = ref.free[:, None]
    structural = int(np.count_nonzero((Y != 0) & ~reach & free))
    passthrough = int(np.count_nonzero((Y != V) & ~free))
    # the probe DOFs of vector c: component[c] of the probe nodes; constrained ones are dropped columns
    fixed3 = ref.fixed.reshape(ref.N, 3)
    dropped = np.asarray(probe_nodes, bool) & fixed3[:, np.asarray(component)]  # [N, m]
    live = ref.reach(np.asarray(probe_nodes, bool) & ~dropped)
    only_dropped = np.repeat(ref.reach(dropped) & ~live, 3, 0)
    leaked = int(np.count_nonzero((Y != 0) & only_dropped & free))
    err = np.abs(Y.astype(np.float64) - Yref) / (U * ref.row_scale[:, None])
    entry = float(np.max(np.where(free, err, 0.0)))
    return dict(structural=structural, passthrough=passthrough, leaked=leaked, entry=entry)


def vector_ratio(ref, x, y):
    """max_i |y - K_ref x|_i / (u (A |x|)_i) over the free rows with a non-zero scale; rows whose scale is 0 must be
    +-0.0 (counted in the second value)."""
    want, scale = ref.apply(x), ref.apply_abs(x)
    err = np.abs(np.asarray(y, np.float64) - want)
    ok = ref.free & (scale > 0)
    ratio = float(np.max(err[ok] / (U * scale[ok]))) if ok.any() else 0.0
    return ratio, int(np.count_nonzero(ref.free & (scale == 0) & (err != 0)))
