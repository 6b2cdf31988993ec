!==========================================================================!
! aggregate_test_hip: the algebraic coarsening through the stand-alone host !
! layer.  The 5-point Poisson matrix of a 63 x 63 grid, the prolongations   !
! of its smoothed-aggregation hierarchy from the matrix alone               !
! (hip_aggregation_hierarchy: theta 0.08, smooth_omega 2/3, at most 25      !
! levels, down to 64 rows), hip_multigrid(P, omega = 0.8) = V(1,1) with 8   !
! coarse sweeps on them, and CG to 1e-10 on b = A x* with and without it.   !
!==========================================================================!
program aggregate_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx0 = 63, ny0 = 63, nn = nx0 * ny0, maxlev = 25
    type(hip_csr_matrix), target :: A
    type(hip_csr_matrix), target :: P(maxlev - 1)
    type(hip_matrix_pointer), allocatable :: Pp(:)
    type(hip_linear_solver), pointer :: solver, plain, pc
    real(dp), allocatable :: xs(:), b(:), u(:)
    integer(c_int32_t), allocatable :: agg(:)
    integer, allocatable :: members(:)
    integer :: ncoarse, nagg, l, i, fails, it_pc, it_plain, levels(2), path, colours
    real(dp) :: est_us
    character(len=96) :: name
    character(len=256) :: line

    fails = 0
    call hip_check(sgm_init(0_c_int))
    call poisson(A, nx0, ny0)

    allocate(agg(nn))
    call hip_aggregate(A, agg, nagg)
    call check('aggregate numbers lie in 1 .. nagg', minval(agg) >= 1 .and. maxval(agg) <= nagg)
    allocate(members(nagg))
    members = 0
    do i = 1, nn
        members(agg(i)) = members(agg(i)) + 1
    enddo
    call check('every aggregate has a member', minval(members) >= 1)
    call check('the grid is reduced at least four times', 4 * nagg <= nn)

    call hip_aggregation_hierarchy(A, P, ncoarse)
    call check('at least two coarse levels', ncoarse >= 2)
    call check('the first prolongation has one column per aggregate', P(1)%nrow == nn .and. P(1)%ncol == nagg)
    do l = 2, ncoarse
        call check('the shapes chain', P(l)%nrow == P(l - 1)%ncol .and. P(l)%ncol < P(l)%nrow)
    enddo
    call check('the last level has at most 64 rows', P(ncoarse)%ncol <= 64)
    write(line, '(a,i0)') ' level sizes ', nn
    do l = 1, ncoarse
        write(line(len_trim(line) + 1:), '(1x,i0)') P(l)%ncol
    enddo
    print '(a)', trim(line)

    allocate(Pp(ncoarse))
    do l = 1, ncoarse
        Pp(l)%mat => P(l)
    enddo

    allocate(xs(nn), b(nn), u(nn))
    do i = 1, nn
        xs(i) = sin(0.001_dp * real(i, dp))
    enddo
    call A%matvec(xs, b)

    pc => hip_multigrid(Pp, omega = 0.8_dp, nu_pre = 1, nu_post = 1, coarse_sweeps = 8)
    call pc%setup(A)
    call pc%info(levels, path, colours, est_us, name)
    print *, 'preconditioner: ', trim(name)
    call check('one level per prolongation and the matrix', levels(1) == ncoarse + 1)

    solver => hip_cg(1.0e-10_dp)
    call solver%setup(A)
    u = 0.0_dp
    call solver%solve(A, u, b, pc)
    it_pc = solver%iterations
    call check('V(1,1)-PCG: max |u - x*| <= 1e-9', maxval(abs(u - xs)) <= 1.0e-9_dp)

    plain => hip_cg(1.0e-10_dp)
    call plain%setup(A)
    u = 0.0_dp
    call plain%solve(A, u, b)
    it_plain = plain%iterations
    call check('plain CG needs more than twice as many iterations', it_plain > 2 * it_pc)
    print '(a,i0)', ' plain CG iterations ', it_plain
    print '(a,i0)', ' V(1,1)-PCG iterations ', it_pc

    call solver%destroy()
    call plain%destroy()
    call pc%destroy()
    ! the prolongations do not depend on the matrix they were made from: it goes first
    call A%destroy()
    do l = 1, ncoarse
        call P(l)%destroy()
    enddo
    if (fails > 0) then
        print *, 'aggregate_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'aggregate_test_hip: ok'

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

end program aggregate_test_hip
