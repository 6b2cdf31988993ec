!==========================================================================!
! mg_direct_test_hip: multigrid's direct coarse solve through the           !
! stand-alone host layer.  The 5-point Poisson matrix of a 63 x 63 grid and !
! only the first two 2:1 interpolations of its grid hierarchy (63, 32, 16): !
! the descent stops at 256 rows.  hip_multigrid(P, omega = 0.8,             !
! coarse_direct = .true.) inverts that level at setup; CG to 1e-10 on       !
! b = A x* with it, and with the 8 coarse sweeps on the same hierarchy.     !
!==========================================================================!
program mg_direct_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx0 = 63, ny0 = 63, nn = nx0 * ny0, nlev = 2
    type(hip_csr_matrix), target :: A
    type(hip_csr_matrix), target :: P(nlev)
    type(hip_matrix_pointer) :: Pp(nlev)
    type(hip_linear_solver), pointer :: solver, solver2, pc, pcs
    real(dp), allocatable :: xs(:), b(:), u(:)
    integer :: nx, ny, l, i, fails, it_direct, it_sweeps, nr, nc, levels(2), path, colours, k
    integer(c_int64_t) :: nnz
    real(dp) :: est_us
    character(len=96) :: name

    fails = 0
    call hip_check(sgm_init(0_c_int))
    call poisson(A, nx0, ny0)
    nx = nx0; ny = ny0
    do l = 1, nlev
        call interp2d(P(l), nx, ny)
        nx = (nx + 1) / 2; ny = (ny + 1) / 2
        Pp(l)%mat => P(l)
    enddo

    allocate(xs(nn), b(nn), u(nn))
    do i = 1, nn
        xs(i) = sin(0.001_dp * real(i, dp))
    enddo
    call A%matvec(xs, b)

    pc => hip_multigrid(Pp, omega = 0.8_dp, nu_pre = 1, nu_post = 1, coarse_sweeps = 8, coarse_direct = .true.)
    call pc%setup(A)
    call pc%info(levels, path, colours, est_us, name)
    print *, 'preconditioner: ', trim(name)
    call check('three levels', levels(1) == nlev + 1)
    call hip_mg_level_info(pc, 2, nr, nc, nnz)
    call check('level 2 is the 16 x 16 grid', nr == 256 .and. nc == 256)
    k = index(trim(name), 'direct coarse solve (256 rows)')
    call check('the name ends with the direct coarse solve and its row count', k > 0 .and. k + 29 == len_trim(name))

    solver => hip_cg(1.0e-10_dp)
    call solver%setup(A)
    u = 0.0_dp
    call solver%solve(A, u, b, pc)
    it_direct = solver%iterations
    call check('direct coarse level: max |u - x*| <= 1e-9', maxval(abs(u - xs)) <= 1.0e-9_dp)
    call check('direct coarse level: at most 14 iterations', it_direct <= 14)

    pcs => hip_multigrid(Pp, omega = 0.8_dp, nu_pre = 1, nu_post = 1, coarse_sweeps = 8, coarse_direct = .false.)
    call pcs%setup(A)
    call pcs%info(levels, path, colours, est_us, name)
    call check('coarse_direct = .false. keeps the sweeps', index(trim(name), '8 coarse sweeps') > 0)
    solver2 => hip_cg(1.0e-10_dp)
    call solver2%setup(A)
    u = 0.0_dp
    call solver2%solve(A, u, b, pcs)
    it_sweeps = solver2%iterations
    call check('8 sweeps on 256 rows need more iterations than the direct solve', it_sweeps > it_direct)
    print '(a,i0)', ' 8-sweep PCG iterations ', it_sweeps
    print '(a,i0)', ' direct PCG iterations ', it_direct

    call solver%destroy()
    call solver2%destroy()
    call pc%destroy()
    call pcs%destroy()
    do l = 1, nlev
        call P(l)%destroy()
    enddo
    call A%destroy()
    if (fails > 0) then
        print *, 'mg_direct_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'mg_direct_test_hip: ok'

contains

subroutine poisson(M, nx, ny)
    type(hip_csr_matrix), intent(inout) :: M
    integer, intent(in) :: nx, ny
    integer :: ptr(nx * ny + 1), k, i, j, e
    integer, allocatable :: node(:)
    real(dp), allocatable :: val(:)
    allocate(node(5 * nx * ny), val(5 * nx * ny))
    e = 0
    do k = 1, nx * ny
        i = mod(k - 1, nx); j = (k - 1) / nx
        ptr(k) = e + 1
        if (j > 0) call put(k - nx, -1.0_dp)
        if (i > 0) call put(k - 1, -1.0_dp)
        call put(k, 4.0_dp)
        if (i < nx - 1) call put(k + 1, -1.0_dp)
        if (j < ny - 1) call put(k + nx, -1.0_dp)
    enddo
    ptr(nx * ny + 1) = e + 1
    call M%init(nx * ny, nx * ny, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
contains
    subroutine put(c, z)
        integer, intent(in) :: c
        real(dp), intent(in) :: z
        e = e + 1
        node(e) = c
        val(e) = z
    end subroutine
end subroutine

! the 2:1 linear interpolation from the coarse grid (the fine points of even i and j, 0-based) to an nx x ny grid
subroutine interp2d(M, nx, ny)
    type(hip_csr_matrix), intent(inout) :: M
    integer, intent(in) :: nx, ny
    integer :: ptr(nx * ny + 1), k, i, j, e, cx, cy, ii(2), jj(2), a, c
    real(dp) :: wi, wj
    integer, allocatable :: node(:)
    real(dp), allocatable :: val(:)
    cx = (nx + 1) / 2; cy = (ny + 1) / 2
    allocate(node(4 * nx * ny), val(4 * nx * ny))
    e = 0
    do k = 1, nx * ny
        i = mod(k - 1, nx); j = (k - 1) / nx
        ptr(k) = e + 1
        call along(i, cx, ii, wi)
        call along(j, cy, jj, wj)
        do a = 1, 2
            do c = 1, 2
                if (jj(a) >= 0 .and. ii(c) >= 0) then
                    e = e + 1
                    node(e) = jj(a) * cx + ii(c) + 1
                    val(e) = wi * wj
                endif
            enddo
        enddo
    enddo
    ptr(nx * ny + 1) = e + 1
    call M%init(nx * ny, cx * cy, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
end subroutine

subroutine along(t, c, idx, w)
    integer, intent(in) :: t, c
    integer, intent(out) :: idx(2)
    real(dp), intent(out) :: w
    idx(1) = t / 2
    idx(2) = -1
    w = 1.0_dp
    if (mod(t, 2) == 1) then
        w = 0.5_dp
        if (t / 2 + 1 < c) idx(2) = t / 2 + 1
    endif
end subroutine

subroutine check(what, ok)
    character(len=*), intent(in) :: what
    logical, intent(in) :: ok
    if (ok) then
        print *, 'ok    ', what
    else
        print *, 'FAILED ', what
        fails = fails + 1
    endif
end subroutine

end program mg_direct_test_hip
