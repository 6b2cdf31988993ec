!==========================================================================!
! lsqr_test_hip: LSQR through the stand-alone host layer.  The case        !
! `fit23x17` of tests/lsqr_restated.py: the 2:1 linear interpolation from  !
! the 12 x 9 coarse grid to the 23 x 17 grid (391 x 108, full column rank),!
! an inconsistent right-hand side read from tests/golden/lsqr/             !
! fit23x17_b.txt (or the file named as the first argument), hip_lsqr(1e-10)!
! from x = 0 with the dot products in sequential order (option dot_order = !
! 1: the count is then pinned).  The solve ends with stop 2: the           !
! least-squares solution, A^T (b - A u) = 0 to the tolerance.              !
!==========================================================================!
program lsqr_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx = 23, ny = 17, cx = (nx + 1) / 2, cy = (ny + 1) / 2, m = nx * ny, n = cx * cy
    type(hip_csr_matrix), target :: A
    type(hip_linear_solver), pointer :: solver
    real(dp), allocatable :: b(:), u(:), q(:), g(:)
    character(len=1024) :: path
    integer :: i, fails, it, ios

    fails = 0
    path = 'tests/golden/lsqr/fit23x17_b.txt'
    if (command_argument_count() >= 1) call get_command_argument(1, path)
    allocate(b(m), u(n), q(m), g(n))
    open(unit=11, file=trim(path), status='old', action='read', iostat=ios)
    if (ios /= 0) then
        print *, 'lsqr_test_hip: cannot open ', trim(path)
        call exit(2)
    endif
    do i = 1, m
        read(11, *) b(i)
    enddo
    close(11)

    call hip_check(sgm_init(0_c_int))
    call interp2d(A)
    solver => hip_lsqr(1.0e-10_dp)
    call solver%set_option("dot_order", 1)
    call solver%setup(A)
    u = 0.0_dp
    call solver%solve(A, u, b)
    it = solver%iterations
    call A%matvec(u, q)
    q = b - q
    call A%matvec_t(q, g)
    call check('LSQR: stop 2, the least-squares solution', solver%stop == 2)
    call check('LSQR: |A^T (b - A u)|_2 <= 2e-10', sqrt(sum(g**2)) <= 2.0e-10_dp)
    call check('LSQR: the residual estimate is the residual', abs(solver%rnorm - sqrt(sum(q**2))) <= 1.0e-10_dp)
    call check('LSQR: fewer than n iterations', it > 0 .and. it < n)
    print '(a,i0)', ' LSQR iterations ', it

    call solver%destroy()
    call A%destroy()
    if (fails > 0) then
        print *, 'lsqr_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'lsqr_test_hip: ok'

contains

subroutine interp2d(M)
    ! problems.interp2d_csr(23, 17): row k = (j, i) of the fine grid takes the coarse points (j/2 [+1], i/2 [+1]) with the
    ! weights 1 (even index) or 1/2 and 1/2 (odd index) along each axis; the columns of a row ascend
    type(hip_csr_matrix), intent(inout) :: M
    integer :: ptr(nx * ny + 1), k, i, j, e, jj, ii, dj, di
    integer, allocatable :: node(:)
    real(dp), allocatable :: val(:)
    real(dp) :: wi, wj
    allocate(node(4 * nx * ny), val(4 * nx * ny))
    e = 0
    do k = 1, nx * ny
        i = mod(k - 1, nx); j = (k - 1) / nx
        ptr(k) = e + 1
        wi = 1.0_dp; wj = 1.0_dp
        if (mod(i, 2) == 1) wi = 0.5_dp
        if (mod(j, 2) == 1) wj = 0.5_dp
        do dj = 0, mod(j, 2)
            jj = j / 2 + dj
            if (jj >= cy) cycle
            do di = 0, mod(i, 2)
                ii = i / 2 + di
                if (ii >= cx) cycle
                e = e + 1
                node(e) = jj * cx + ii + 1
                val(e) = wi * wj
            enddo
        enddo
    enddo
    ptr(nx * ny + 1) = e + 1
    call M%init(nx * ny, cx * cy, ptr, node(1:e))
    M%val = val(1:e)
    M%values_dirty = .true.
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

end program lsqr_test_hip
