!==========================================================================!
! eigsh_test_hip: extreme eigenpairs through the stand-alone host layer.    !
! tridiag(-1, 2, -1) of order 127 (eigenvalues 2 - 2 cos(j pi / 128), all   !
! simple), hip_eigsh for the 4 smallest with ncv = 20 and tol = 1e-10 from  !
! the default start vector.  Prints every eigenvalue with the residual norm !
! the library reports, the one this program forms itself with A%matvec,     !
! and |v|_2, at full precision: tests/test_gpu_eigsh.py reads them.         !
!==========================================================================!
program eigsh_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nn = 127, k = 4
    real(dp), parameter :: pi = 3.14159265358979323846264338327950288_dp
    type(hip_csr_matrix), target :: A
    real(dp) :: lambda(k), V(nn, k), resid(k), q(nn), own, exact
    integer :: ptr(nn + 1), node(3 * nn), i, e, fails, restarts, products, found
    real(dp) :: val(3 * nn)
    logical :: converged

    fails = 0
    call hip_check(sgm_init(0_c_int))
    e = 0
    do i = 1, nn
        ptr(i) = e + 1
        if (i > 1) call put(i - 1, -1.0_dp)
        call put(i, 2.0_dp)
        if (i < nn) call put(i + 1, -1.0_dp)
    enddo
    ptr(nn + 1) = e + 1
    call A%init(nn, nn, ptr, node(1:e))
    A%val = val(1:e)
    A%values_dirty = .true.

    call hip_eigsh(A, k, 'SA', lambda, V=V, resid=resid, ncv=20, tol=1.0e-10_dp, restarts=restarts, products=products, &
        & found=found, converged=converged)
    call check('eigsh: converged with 4 pairs', converged .and. found == k)
    print '(a,i0,a,i0)', ' EIGSH restarts ', restarts, ' products ', products
    do i = 1, k
        call A%matvec(V(:, i), q)
        own = sqrt(sum((q - lambda(i) * V(:, i))**2))
        exact = 2.0_dp - 2.0_dp * cos(real(i, dp) * pi / 128.0_dp)
        print '(a,i0,4(1x,es24.16e3))', ' EIGSH pair ', i, lambda(i), resid(i), own, sqrt(sum(V(:, i)**2))
        call check('eigsh: eigenvalue within 1e-9 of 2 - 2 cos(j pi / 128)', abs(lambda(i) - exact) <= 1.0e-9_dp)
    enddo

    call A%destroy()
    if (fails > 0) then
        print *, 'eigsh_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'eigsh_test_hip: ok'

contains

subroutine put(c, z)
    integer, intent(in) :: c
    real(dp), intent(in) :: z
    e = e + 1
    node(e) = c
    val(e) = z
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

end program eigsh_test_hip
