!==========================================================================!
! minres_test_hip: MINRES through the stand-alone host layer.  The 5-point  !
! Poisson matrix of a 24 x 24 grid with 0.3 subtracted from every diagonal  !
! entry -- symmetric and indefinite: CG is undefined on it --,              !
! b(i) = sin(0.001 i), hip_minres(1e-10) from x = 0 with the dot products   !
! in sequential order (option dot_order = 1: the count is then pinned).     !
!==========================================================================!
program minres_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx = 24, ny = 24, nn = nx * ny
    type(hip_csr_matrix), target :: A
    type(hip_linear_solver), pointer :: solver
    real(dp), allocatable :: b(:), u(:), q(:)
    integer :: i, fails, it

    fails = 0
    call hip_check(sgm_init(0_c_int))
    call shifted_poisson(A, nx, ny, 0.3_dp)
    allocate(b(nn), u(nn), q(nn))
    do i = 1, nn
        b(i) = sin(0.001_dp * real(i, dp))
    enddo

    solver => hip_minres(1.0e-10_dp)
    call solver%set_option("dot_order", 1)
    call solver%setup(A)
    u = 0.0_dp
    call solver%solve(A, u, b)
    it = solver%iterations
    call A%matvec(u, q)
    call check('MINRES: |b - A u|_2 <= 2e-10', sqrt(sum((b - q)**2)) <= 2.0e-10_dp)
    call check('MINRES: fewer than n iterations', it > 0 .and. it < nn)
    print '(a,i0)', ' MINRES iterations ', it

    call solver%destroy()
    call A%destroy()
    if (fails > 0) then
        print *, 'minres_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'minres_test_hip: ok'

contains

subroutine shifted_poisson(M, nx, ny, shift)
    type(hip_csr_matrix), intent(inout) :: M
    integer, intent(in) :: nx, ny
    real(dp), intent(in) :: shift
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
        call put(k, 4.0_dp - shift)
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

end program minres_test_hip
